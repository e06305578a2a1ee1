// vf.inl -- the visual feedback integrator (included by render.hip, translation unit 0, after ao.inl; shares every device function above it).
//
// IntVFInstance::handleShadingGroup and onTile (src/plugins/main/integrators/visualfeedback.cpp:108-233, :235-250): the debug view of a
// camera sample's first hit.  Nothing is drawn from the pixel's generator after the camera sample (the Random(42) of :111 only feeds
// validate_material, which is not built), there are no shadow and no bounce rays, and a hit splats ONE fragment
// pushSpectralFragment(Ones, Ones, radiance, ray) (:231) whose radiance is a fixed colour -- prepared once by the default upsampler, here
// the coefficient rows of VfState::colours, and evaluated at the sample's four wavelengths by upsample() -- times a quantity of the hit.
//
// One iteration = k_raygen -> k_trace_closest (both as for `direct`) -> k_vf_shade -> k_resolve: no hit queue, no second traversal.
//
// The quirks this file follows:
//   * NdotV = dot(ray direction, N) (IntersectionPoint.h:71): negative for a front face, and N is never flipped towards the viewer.
//   * CameraDepthCount counts every shading group, the background ones included (:243) -- `ao` counts hits only (ambientocclusion.cpp:34).
//   * An absent material / emission id is PR_INVALID_ID and 0xFFFFFFFF % 23 = 11; GeometryPoint::DisplaceID is never set by any entity
//     (GeometryPoint.h:24, "TODO") and starts as PR_INVALID_ID, so colored_displace_id is colour 11 on every hit.
//   * `ndotv` is never weighted (:188-197); every other mode is multiplied by |NdotV| when :weighting is on (:126-127 ...).
//   * HitEntry::Parameter is (u, v, t) of the intersector (ShadingGroup.cpp:48-50): the triangle's barycentrics for a mesh, the quad's
//     parameters for a plane (plane.cpp:214, as geometry_point restates them), and u = v = 0 for spheres, quadrics (quadric.cpp:169-170) and disks.

// SpectralUpsampler::compute (SpectralUpsampler.h:45-49) of colour row `c` at the sample's wavelengths.  The row index differs per lane
// (id % 23): the rows live in a small device buffer, one 16-byte load per lane, never in an array indexed at run time.
__device__ __forceinline__ Blob vf_colour(const VfState& vf, uint32_t c, const Blob& wl)
{
	const float4 k	 = vf.colours[c];
	const float p[3] = { k.x, k.y, k.z };
	return blob4(upsample(p, wl.v[0]), upsample(p, wl.v[1]), upsample(p, wl.v[2]), upsample(p, wl.v[3]));
}
// r * a + g * b + b * c per wavelength, summed left to right as the reference's expression (:169, :177)
__device__ __forceinline__ Blob vf_rgb_mix(const VfState& vf, const Blob& wl, float a, float b, float c)
{
	const Blob R = vf_colour(vf, VF_RED, wl), G = vf_colour(vf, VF_GREEN, wl), B = vf_colour(vf, VF_BLUE, wl);
	Blob out;
	for (int k = 0; k < 4; ++k)
		out.v[k] = (R.v[k] * a + G.v[k] * b) + B.v[k] * c;
	return out;
}

// One thread per slot: the whole first vertex of the camera sample -- statistics, geometry point, primary-hit planes and shading-point
// commit (camera_vertex, shared with k_ao_hits), the mode's radiance, and the fragment through the splat path every `direct` fragment takes.
__global__ void __launch_bounds__(256) k_vf_shade(DevScene sc, PathState ps, VfState vf, uint32_t n_slots, uint32_t* queue_head_closest, unsigned long long* gstats)
{
	__shared__ BlockStats bs;
	stats_init(bs);
	if (blockIdx.x == 0 && threadIdx.x == 0) // no traversal launch is in flight during this pass
		*queue_head_closest = 0;
	const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
	CameraVertex cv;
	const int what = camera_vertex(sc, ps, slot, n_slots, bs, cv);
	if (what != CV_NONE)
		atomicAdd(&bs.v[PRGPU_STAT_CAMERA_DEPTH], 1u); // every shading group, background or not (:243)
	if (what == CV_HIT) {
		const Blob wl	   = from4(ps.st[slot].wl);
		const float ndotv  = dot(cv.ray_d, cv.gp.N);
		const float weight = fabsf(ndotv);
		bool weighted	   = vf.weighting != 0u;
		Blob radiance;
		switch (vf.mode) { // uniform over the launch
		case PRGPU_VF_COLORED_ENTITY_ID: radiance = vf_colour(vf, cv.gp.entity % VF_RANDOM_COLOURS, wl); break;
		case PRGPU_VF_COLORED_MATERIAL_ID: radiance = vf_colour(vf, cv.gp.material % VF_RANDOM_COLOURS, wl); break;
		case PRGPU_VF_COLORED_EMISSION_ID: radiance = vf_colour(vf, cv.gp.emission % VF_RANDOM_COLOURS, wl); break;
		case PRGPU_VF_COLORED_DISPLACE_ID: radiance = vf_colour(vf, INVALID % VF_RANDOM_COLOURS, wl); break;
		case PRGPU_VF_COLORED_PRIMITIVE_ID: radiance = vf_colour(vf, cv.gp.prim % VF_RANDOM_COLOURS, wl); break;
		case PRGPU_VF_RAY_DIRECTION: // 0.5 * (direction + 1) (:165)
			radiance = vf_rgb_mix(vf, wl, 0.5f * (cv.ray_d.x + 1.0f), 0.5f * (cv.ray_d.y + 1.0f), 0.5f * (cv.ray_d.z + 1.0f));
			break;
		case PRGPU_VF_PARAMETER: {
			const uint32_t kind = sc.entities[cv.gp.entity].kind;
			const bool planar	= kind == PRGPU_ENTITY_MESH || kind == PRGPU_ENTITY_PLANE;
			const float u = kind == PRGPU_ENTITY_PLANE ? cv.gp.uv[0] : cv.hit4.y, v = kind == PRGPU_ENTITY_PLANE ? cv.gp.uv[1] : cv.hit4.z;
			radiance = vf_rgb_mix(vf, wl, planar ? u : 0.0f, planar ? v : 0.0f, cv.hit4.x);
		} break;
		case PRGPU_VF_INSIDE: radiance = vf_colour(vf, !signbit(ndotv) ? VF_GREEN : VF_RED, wl); break; // True / False (:183)
		default: // PRGPU_VF_NDOTV (:188-197)
			radiance = ndotv < 0 ? vf_colour(vf, VF_GREEN, wl) * (-ndotv) : vf_colour(vf, VF_RED, wl) * ndotv;
			weighted = false;
			break;
		}
		if (weighted)
			radiance = radiance * weight;
		const uint32_t flags = ps.st[slot].flags;
		const PathCie cie	 = slot_cie(ps, slot);
		const Blob grp_imp	 = (flags & FLAG_GROUP_MONO) ? hero_only() : blob(1.0f); // RenderTile.cpp:126-127 (importance of the ray group)
		float xyz[3];
		const uint32_t fb = fragment_value(sc, blob(1), blob(1), grp_imp, radiance, (flags & FLAG_MONO) != 0, cie, 1.0f, xyz);
		apply_fragment(ps, cv.pixel, iter_entry(ps, slot, cv.pixel), fb, xyz);
	}
	stats_flush(bs, gstats);
}
