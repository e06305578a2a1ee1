// ao.inl -- the ambient occlusion integrator (included by render.hip, translation unit 0; shares every device function above it).
//
// IntAOInstance::handleShadingGroup (src/plugins/main/integrators/ambientocclusion.cpp:29-74): a camera sample that hits a surface draws
// `sample_count` directions from the UNIFORM hemisphere around the shading normal (Sampling::hemi, base/math/Sampling.h:23-29) with the
// pixel's generator, asks traceShadowRay for each (interval [PR_EPSILON, inf), RenderTileSession.cpp:103-111, IArchive.h:21) and splats
// weight = 1 - occlusions / sample_count on all four wavelengths with unit importance; a miss counts a background hit and nothing else.
//
// One iteration = k_raygen -> k_trace_closest (both as for `direct`) -> k_ao_hits -> k_ao_occlusion -> k_ao_splat -> k_resolve.
//   * k_ao_hits: statistics, geometry_point, the shading-point commit of direct's first vertex, and ONE 64-byte record per hit (P, N, Nx, Ny,
//     the slot, the generator state before the first AO draw), compacted with wave_append.  The random budget of a hit is fixed -- 2 N
//     draws whatever the rays find -- and the generator is a multiplicative congruential one (pr_device.h, rng_u32: state *= PCG_MULT per
//     draw), so the pixel's stream moves on by one multiplication with PCG_MULT^(2 N) right here, and sample k of a hit starts from
//     state * PCG_MULT^(2 k): no ray waits for the one before it.
//   * k_ao_occlusion: trace_persistent<any hit> over n_hits x N VIRTUAL rays -- ray i is sample i % N of hit i / N, built in the lane that
//     picks it up from the hit's record and a table of PCG_MULT^(2 k); nothing is stored per ray.  The N rays of a hit are neighbours in
//     the queue: they share an origin and walk the same part of the tree.
//   * k_ao_splat: weight, the counts plane, and the fragment through the splat path every `direct` fragment takes.
#ifndef PR_AO_FOLD
#define PR_AO_FOLD 1 // finished rays of one hit in a wave step add their occluded bits with ONE atomic (ballot + popcount); 0: one atomic per occluded ray
#endif

// Sampling::hemi (base/math/Sampling.h:23-29): uniform over the hemisphere around +z, u1 is the cosine
__device__ __forceinline__ V3 uniform_hemi(float u1, float u2)
{
	const float sinTheta = sqrtf(fmaxf(0.0f, 1.0f - u1 * u1));
	float s, c;
	pr_sincos_2pi(u2, s, c);
	return v3(sinTheta * c, sinTheta * s, u1);
}

// The camera rays' hits: handleShadingGroup up to the sample loop (ambientocclusion.cpp:33-38) and onTile's background branch (:68-69) --
// camera_vertex (render.hip), which k_vf_shade shares -- and the hit's record.
template <bool INSTR>
__global__ void __launch_bounds__(256) k_ao_hits(DevScene sc, PathState ps, AoState ao, uint32_t n_slots, uint32_t* __restrict__ n_hits /* zeroed by k_trace_closest */,
												 uint32_t* queue_head_closest, uint32_t* queue_head_ao, unsigned long long* gstats)
{
	__shared__ BlockStats bs;
	stats_init(bs);
	if (blockIdx.x == 0 && threadIdx.x == 0) { // no traversal launch is in flight during this pass
		*queue_head_closest = 0;
		*queue_head_ao		= 0;
	}
	const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
	bool hit			= false;
	float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0, r3 = r0;
	CameraVertex cv;
	if (camera_vertex(sc, ps, slot, n_slots, bs, cv) == CV_HIT) { // (statistics of hit and background, geometry point, primary-hit planes, pushSPFragment (:55))
		const uint32_t pixel = cv.pixel;
		const V3 P			 = cv.P;
		const GeomPoint& gp	 = cv.gp;
		atomicAdd(&bs.v[PRGPU_STAT_CAMERA_DEPTH], 1u); // hits only (:34)
		atomicAdd(&bs.v[PRGPU_STAT_SHADOW_RAYS], ao.sample_count);
		const uint64_t state = ps.rng[pixel];
		ps.rng[pixel]		 = state * ao.jump_all; // 2 N draws, whatever the rays find
		if (INSTR)
			ao.dbg_state[pixel] = state;
		r0	= make_float4(P.x, P.y, P.z, __uint_as_float(slot));
		r1	= make_float4(gp.N.x, gp.N.y, gp.N.z, __uint_as_float((uint32_t)state));
		r2	= make_float4(gp.Nx.x, gp.Nx.y, gp.Nx.z, __uint_as_float((uint32_t)(state >> 32)));
		r3	= make_float4(gp.Ny.x, gp.Ny.y, gp.Ny.z, 0.0f);
		hit = true;
	}
	const uint32_t h = wave_append(hit, n_hits);
	if (hit) {
		ao.rec[4 * size_t(h) + 0] = r0;
		ao.rec[4 * size_t(h) + 1] = r1;
		ao.rec[4 * size_t(h) + 2] = r2;
		ao.rec[4 * size_t(h) + 3] = r3;
		ao.occluded[h]			  = 0u;
	}
	stats_flush(bs, gstats);
}

// The sample loop (ambientocclusion.cpp:41-51) for every hit at once.  INSTR: traversal counters and the ray dump of prgpu_download_ao_samples.
template <bool INSTR>
__global__ void __launch_bounds__(TRAV_BLOCK) k_ao_occlusion(DevScene sc, PathState ps, AoState ao, const uint32_t* __restrict__ n_hits, uint32_t* queue_head, uint2* spill,
															int refill_below, unsigned long long* gstats)
{
	const uint32_t N	  = ao.sample_count;
	const uint32_t n_rays = *n_hits * N; // (the host sized the grid for every owned pixel hitting: no read-back between the passes)
	auto load = [&](uint32_t i, V3& o, V3& d, float& tmin, float& tmax) {
		const uint32_t h = i / N, k = i - h * N;
		const float4 r0 = ao.rec[4 * size_t(h)], r1 = ao.rec[4 * size_t(h) + 1], r2 = ao.rec[4 * size_t(h) + 2], r3 = ao.rec[4 * size_t(h) + 3];
		uint64_t rnd   = ((uint64_t(__float_as_uint(r2.w)) << 32) | __float_as_uint(r1.w)) * ao.jump[k];
		const float u1 = rng_float(rnd); // random.get2D(): u1 first (:42)
		const float u2 = rng_float(rnd);
		const V3 P = v3(r0.x, r0.y, r0.z), Ng = v3(r1.x, r1.y, r1.z);
		d	 = from_tangent_space(Ng, v3(r2.x, r2.y, r2.z), v3(r3.x, r3.y, r3.z), uniform_hemi(u1, u2));
		o	 = safe_position(P, d, Ng); // Ray::next with a normal (ray/Ray.h:118-122)
		tmin = PR_EPS;
		tmax = INFINITY;
		if (INSTR) {
			const size_t e = size_t(ps.pixel[__float_as_uint(r0.w)]) * N + k;
			ao.dbg_org[3 * e] = o.x; ao.dbg_org[3 * e + 1] = o.y; ao.dbg_org[3 * e + 2] = o.z;
			ao.dbg_dir[3 * e] = d.x; ao.dbg_dir[3 * e + 1] = d.y; ao.dbg_dir[3 * e + 2] = d.z;
		}
	};
	auto store = [&](uint32_t i, const Hit& hit) { // called by the lanes whose ray ended in this wave step
		const uint32_t h = i / N;
		const bool occ	 = hit.tri != INVALID;
		if (INSTR)
			ao.dbg_occluded[size_t(ps.pixel[__float_as_uint(ao.rec[4 * size_t(h)].w)]) * N + (i - h * N)] = occ ? 1 : 0;
#if PR_AO_FOLD
		unsigned long long todo = lane_ballot(occ);
		while (todo != 0ull) { // one round per hit among the occluded lanes (the rays of a hit are queue neighbours: one or two rounds)
			const uint32_t h0			   = (uint32_t)__builtin_amdgcn_readlane((int)h, __builtin_ctzll(todo));
			const unsigned long long same = lane_ballot(occ && h == h0);
			if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(same))
				atomicAdd(&ao.occluded[h0], (uint32_t)__builtin_popcountll(same));
			todo &= ~same;
		}
#else
		if (occ)
			atomicAdd(&ao.occluded[h], 1u);
#endif
	};
	trace_persistent<true, INSTR>(sc, n_rays, queue_head, spill, refill_below, load, store, gstats);
}

// weight = 1 - occlusions / N and pushSpectralFragment(Ones, Ones, weight, ray) (ambientocclusion.cpp:53-56)
__global__ void __launch_bounds__(256) k_ao_splat(DevScene sc, PathState ps, AoState ao, const uint32_t* __restrict__ n_hits)
{
	const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
	if (h >= *n_hits)
		return;
	const uint32_t slot	 = __float_as_uint(ao.rec[4 * size_t(h)].w);
	const uint32_t pixel = ps.pixel[slot];
	const uint32_t occ	 = ao.occluded[h];
	ao.counts[pixel] += occ;
	const float weight	 = 1.0f - occ / (float)ao.sample_count;
	const uint32_t flags = ps.st[slot].flags;
	const PathCie cie  = slot_cie(ps, slot);
	const Blob grp_imp = (flags & FLAG_GROUP_MONO) ? hero_only() : blob(1.0f); // RenderTile.cpp:126-127 (importance of the ray group)
	float xyz[3];
	const uint32_t fb = fragment_value(sc, blob(1), blob(1), grp_imp, blob(weight), (flags & FLAG_MONO) != 0, cie, 1.0f, xyz);
	apply_fragment(ps, pixel, iter_entry(ps, slot, pixel), fb, xyz);
}
