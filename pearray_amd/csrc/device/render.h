// render.h -- host-callable launchers of the wavefront kernels (render.hip).
#pragma once
#include "pr_device.h"

namespace prd {
// gstats: PRGPU_STAT_COUNT statistics, then inner/leaf record counters of closest and any-hit traversal, then wave-iteration
// counters, then the persistent kernel's shading passes / shaded vertices / time split
constexpr int N_DEVICE_COUNTERS = PRGPU_STAT_COUNT + 32; // ... + diagnostics (PRGPU_DEBUG_COUNTERS): leaf-step / inner-step ticks, shader cycles, refill ticks, ray-end ticks

// Scratch of one persistent traversal launch: queue head (u32) and the per-thread stack spill slab.
// Launches that may run concurrently need separate workspaces.
struct TraceWorkspace {
	uint32_t* queue_head = nullptr;
	uint2* spill		 = nullptr; // max_blocks * 256 * STACK_SPILL entries
	uint32_t max_blocks	 = 0;		// persistent grid size (blocks)
	int refill_below	 = 44;		// refill a wave from the queue when fewer lanes than this are active
	// persistent path kernel, resident pixels: per-block pixel lists and state words (bl_entries each), per-slot list index
	uint32_t* bl_list	 = nullptr;
	uint32_t* bl_word	 = nullptr;
	uint32_t* slot_unit	 = nullptr;
	size_t bl_entries	 = 0;
};
size_t trace_workspace_spill_entries(uint32_t max_blocks);
uint32_t trace_stack_capacity(); // entries a lane's traversal stack holds (LDS window + spill slab)

// slot_base: first slot of the pixel group when `active` is null (identity list of the primary wave)
void launch_raygen(const DevScene& sc, const PathState& ps, uint32_t slot_base, uint32_t n_slots, uint32_t iter, unsigned long long* gstats, hipStream_t st);
void launch_trace_closest(const DevScene& sc, const PathState& ps, const uint32_t* active, uint32_t slot_base, uint32_t n_active, bool count,
						  const TraceWorkspace& ws, uint32_t* shade_counters, unsigned long long* gstats, hipStream_t st);
// shade also clears the two queue heads for the next traversal launches of the group
// counters: [0] survivors appended to next_active, [1] shadow-queue items, [2] paths ended (appended to dead_list when it is non-null)
void launch_shade(const DevScene& sc, const PathState& ps, const uint32_t* active, uint32_t slot_base, uint32_t n_active, uint32_t* next_active,
				  uint32_t* counters, uint32_t* dead_list, uint32_t* queue_head_closest, uint32_t* queue_head_shadow, unsigned long long* gstats,
				  hipStream_t st);
// streaming mode: fold finished paths into the running mean and start the pixel's next sample (appends to next_active / counters[0])
void launch_regen(const DevScene& sc, const PathState& ps, const uint32_t* dead, uint32_t n_dead, uint32_t iter_end, uint32_t* next_active,
				  uint32_t* counters, unsigned long long* gstats, hipStream_t st);
void launch_trace_shadow(const DevScene& sc, const PathState& ps, uint32_t n_items, bool count, const TraceWorkspace& ws, unsigned long long* gstats,
						 hipStream_t st);
// Persistent path kernel (single-tap filters): the whole render call [iter_begin, iter_end) of the `n_owned` pixels of `owned`
// in one launch.  ps.pixel must be a per-slot scratch array (NOT the owned list) of n_blocks * slots_per_block entries.
struct PersistentGeometry {
	uint32_t n_blocks, slots_per_block;
};
PersistentGeometry persistent_geometry(uint32_t n_owned, uint32_t max_blocks, uint32_t max_slots_per_block);
uint32_t persistent_slot_padding(); // slots per block of the throughput kernel at most (PRGPU_PP_SLOTS is clamped to it)
uint32_t slot_array_padding();	   // per-slot arrays need n_pixels + this many entries (either organisation rounds its slot count up)
uint32_t persistent_block_threads(); // 256 or 768 (PR_PP_BLOCK)
int shade_ticks_counter(); // index into gstats of the instrumented kernel's timers: ticks in shading passes, idle, alive (summed over waves)
// What a host may tune in the persistent kernel without changing a result (prgpu_api.hip reads the PRGPU_PP_* knobs into this)
struct PersistentTuning {
	uint32_t slots	  = 384; // path slots per block of 256 lanes (256 .. 512; round 4: 384 is 3 % faster than 512 on C4, profiles/r04_knobs.log)
	int shade_min	  = 64;	 // a shading pass starts once this many vertices of one class wait ...
	int shade_partial = 16;	 // ... or this many when no ray is queued and the wave is short of rays anyway
	int fin_batch	  = 16;	 // finished rays are written out once this many lanes of a wave hold one
	int occupancy	  = 3;	 // waves per SIMD the kernel variant is compiled for (3: 168 VGPRs, 2: 256)
	int shader_wave	  = -1;	 // 0 .. 2: dedicated shading waves per block; -1: one when every owned pixel is in flight at once, else by the
							 // measured share of shading in the wave time of the scene's first launch (prgpu_api.hip, render_persistent)
	bool resident	  = true; // pixels stay with a block, not with a slot (off: a slot keeps its pixel for all samples of a launch)
};
void launch_path_persistent(const DevScene& sc, const PathState& ps, const uint32_t* owned, uint32_t n_owned, uint32_t iter_begin, uint32_t iter_end,
							bool count, const TraceWorkspace& ws, const PersistentTuning& tune, int shader_waves /* of a block's four: 0 .. 2 */, uint32_t* next_pixel, uint32_t* error,
							unsigned long long* gstats, hipStream_t st);
// The compiled variants of the path kernel (either organisation), in order of preference: a scene runs the FIRST row whose mask covers its
// features -- lean (Lambert / mesh / area lights), + smooth delta materials, everything but the rough / principled closures, everything but
// light path expressions, everything.  The out-of-line closures are what the fourth row pays for: a kernel that CONTAINS the calls runs a
// scene that never makes them 25 % slower (metal Cornell box: 3.18 vs 4.02 ms per iteration; leaving out spheres, AOVs + textures or
// infinite / shape lights + planes instead changes nothing).  A variant for delta + rough materials only was measured and dropped: the
// closures dominate such scenes, 156 vs 154 Msamples/s.  Light path expressions are a row of their own because their state tracking costs
// the all-features kernel 7 % (C5 135 -> 125 Msamples/s); quadric and disk entities, image textures (FEAT_IMAGES) and the Oren-Nayar / null / blend / add
// materials (FEAT_MIX_MATERIALS) ride in that top row (what a disk or an image scene pays for the expression hooks there has not been measured).
// Spectral expression roots (FEAT_EXPR) ride there too, in exactly the rows that have FEAT_IMAGES: the closures'
// _uv forms (rough_closures.inl) serve both.  Scalar nodes on scalar material parameters (FEAT_SCALAR_NODES) ride in
// the top row alone: scalar_resolve writes a vertex's resolved values into its local material record, which the closures read as before.
// A translation unit of render.hip takes its row by -DPR_VARIANT=<id>.  Adding a variant takes exactly two edits: a row here, and its id in
// the Makefile's VARIANTS list.
struct PathVariant {
	int id;			   // PR_VARIANT of its translation units; bit id - 1 of PR_PL_VARIANTS
	uint32_t features; // FEAT_* bits the kernel is compiled with
};
constexpr uint32_t FEAT_NO_LPE = FEAT_ALL & ~(FEAT_LPE | FEAT_QUADRICS | FEAT_DISKS | FEAT_IMAGES | FEAT_MIX_MATERIALS | FEAT_EXPR | FEAT_SCALAR_NODES), FEAT_NO_ROUGH = FEAT_NO_LPE & ~FEAT_ROUGH_MATERIALS;
constexpr PathVariant PATH_VARIANTS[] = { { 1, 0u }, { 2, FEAT_DELTA_MATERIALS }, { 3, FEAT_NO_ROUGH }, { 4, FEAT_NO_LPE }, { 5, FEAT_ALL } };
constexpr int N_PATH_VARIANTS		  = int(sizeof(PATH_VARIANTS) / sizeof(PATH_VARIANTS[0]));
// index of the scene's row
constexpr int path_variant(uint32_t features)
{
	for (int i = 0; i < N_PATH_VARIANTS - 1; ++i)
		if ((features & ~PATH_VARIANTS[i].features) == 0u)
			return i;
	return N_PATH_VARIANTS - 1;
}
// index of the row with this id (N_PATH_VARIANTS: none)
constexpr int path_variant_row(int id)
{
	int i = 0;
	while (i < N_PATH_VARIANTS && PATH_VARIANTS[i].id != id)
		++i;
	return i;
}
constexpr bool path_variants_nested()
{
	for (int i = 0; i + 1 < N_PATH_VARIANTS; ++i)
		if ((PATH_VARIANTS[i].features & ~PATH_VARIANTS[i + 1].features) != 0u)
			return false;
	return true;
}
static_assert(PATH_VARIANTS[N_PATH_VARIANTS - 1].features == FEAT_ALL, "the last variant must cover every scene");
constexpr bool expr_rides_with_images()
{
	for (int i = 0; i < N_PATH_VARIANTS; ++i)
		if (((PATH_VARIANTS[i].features & FEAT_IMAGES) != 0u) != ((PATH_VARIANTS[i].features & FEAT_EXPR) != 0u))
			return false;
	return true;
}
static_assert(expr_rides_with_images(), "FEAT_EXPR and FEAT_IMAGES must sit in the same rows: the closures' _uv forms serve both");
static_assert(path_variants_nested(), "each variant's mask must be contained in the next one's: then the first covering row is the smallest covering one");
// The throughput organisation compiles every variant in these forms (its sub-units, -DPR_SUB=<index>): for 3 waves per SIMD with four-
// or six-wide inner records, or for 2 waves per SIMD (one kernel for both widths), each plain and instrumented (COUNT).
struct PathSub {
	int occupancy;
	bool wide, count;
};
constexpr PathSub PATH_SUBS[] = { { 3, false, false }, { 3, false, true }, { 2, false, false }, { 2, false, true }, { 3, true, false }, { 3, true, true } };
constexpr int N_PATH_SUBS	  = int(sizeof(PATH_SUBS) / sizeof(PATH_SUBS[0]));
// index of the sub-unit that serves a launch (N_PATH_SUBS: none)
constexpr int path_sub(int occupancy, bool wide, bool count)
{
	const int occ = occupancy >= 3 ? 3 : 2;
	int i		  = 0;
	while (i < N_PATH_SUBS && !(PATH_SUBS[i].occupancy == occ && PATH_SUBS[i].count == count && (occ == 2 || PATH_SUBS[i].wide == wide)))
		++i;
	return i;
}
constexpr bool path_subs_complete()
{
	for (int k = 0; k < 8; ++k) // every (occupancy, wide, count) has a sub-unit ...
		if (path_sub(2 + (k >> 2), (k & 2) != 0, (k & 1) != 0) >= N_PATH_SUBS)
			return false;
	for (int i = 0; i < N_PATH_SUBS; ++i) // ... and every sub-unit is the one its own row selects
		if (path_sub(PATH_SUBS[i].occupancy, PATH_SUBS[i].wide, PATH_SUBS[i].count) != i)
			return false;
	return true;
}
static_assert(path_subs_complete(), "PATH_SUBS and path_sub disagree");
// The latency organisation of the same kernel (device/path_wave.inl): a WAVE owns 64 .. 256 path slots with wave-private queues, two blocks
// per CU at two waves per SIMD -- for tile shares whose pixel count is about the chip's lane count, where a launch lasts as long as its
// deepest pixel's chain of vertices.  Same frame, bit for bit.  Measured slower there than the throughput organisation,
// so nothing selects it by default: PRGPU_PP_KERNEL=auto always runs the throughput kernel, and only PRGPU_PP_KERNEL=latency runs this one.
struct LatencyGeometry {
	uint32_t n_blocks, slots_per_wave, total_slots;
};
struct LatencyTuning {
	uint32_t slots_per_wave = 256; // cap; the launcher takes the smallest multiple of 64 that puts every owned pixel in flight
	int shade_min			= 48;  // a shading pass starts once this many vertices of one class wait ...
	int refill_below		= 40;  // ... or when fewer lanes than this hold a running ray and nothing is queued for the idle ones
};
LatencyGeometry latency_geometry(uint32_t n_owned, uint32_t max_blocks_throughput, uint32_t max_slots_per_wave);
bool latency_variant_built(uint32_t features);
void launch_path_latency(const DevScene& sc, const PathState& ps, const uint32_t* owned, uint32_t n_owned, uint32_t iter_begin, uint32_t iter_end, bool count,
						 const TraceWorkspace& ws, const LatencyTuning& tune, uint32_t* error, unsigned long long* gstats, hipStream_t st);
void launch_resolve(const DevScene& sc, const PathState& ps, uint32_t iter, hipStream_t st);
// lockstep pipeline, PRGPU_SORT_RAYS=1 (experiment): the active list ordered by (Morton code of the ray origin, direction octant)
size_t sort_active_temp_bytes(uint32_t n_max);
void launch_sort_active(const DevScene& sc, const PathState& ps, const uint32_t* active, uint32_t n, uint32_t* keys_in, uint32_t* keys_out, uint32_t* active_out,
						void* temp, size_t temp_bytes, hipStream_t st);
void launch_service_closest(const DevScene& sc, uint32_t n, const float* org, const float* dir, const float* tmin, const float* tmax,
							uint32_t* entity, uint32_t* prim, float* u, float* v, float* t, const TraceWorkspace& ws, unsigned long long* gstats,
							hipStream_t st);
void launch_tri_slot(const DevScene& sc, const uint32_t* leaf_units /* unit of every leaf record (BvhBuildOutput) */, uint32_t* tri_slot, hipStream_t st); // fills DevScene::tri_slot from the leaf records
void launch_service_closest_split(const DevScene& sc, uint32_t n, const float* org, const float* dir, const float* tmin, const float* tmax,
								  uint32_t* entity, uint32_t* prim, float* u, float* v, float* t, const TraceWorkspace& ws, uint32_t* tri_slot,
								  unsigned long long* gstats, bool leaf_single /* the tree's leaves are single leaves */, hipStream_t st); // prototype, see render.hip
void launch_service_any(const DevScene& sc, uint32_t n, const float* org, const float* dir, const float* tmin, const float* distance,
						uint8_t* occluded, const TraceWorkspace& ws, unsigned long long* gstats, hipStream_t st);
// The ray service on caller-owned DEVICE memory (prgpu_trace_closest_device / prgpu_trace_any_device): the same traversal kernels, compiled with
// the refused-ray rule (a ray with !(tmin >= 0) is a miss and counts in *invalid) and a NULL test per output, and the geometry pass behind them.
struct ServiceRays {
	uint32_t n;
	const float *org, *dir, *tmin, *tmax; // tmax: the distance of an occlusion ray
};
struct ServiceHits { // every pointer may be null, except -- for launch_service_geometry -- tri, u, v, t, which it reads
	uint32_t *entity, *prim;
	float *u, *v, *t;
	uint32_t* tri; // the winning triangle's scene-wide index (INVALID on a miss)
	float *position, *normal, *tangent, *bitangent, *uv;
	uint32_t *material, *emission, *invalid;
};
void launch_service_closest_device(const DevScene& sc, const ServiceRays& r, const ServiceHits& h, bool split, const TraceWorkspace& ws, uint32_t* tri_slot,
								   unsigned long long* gstats, bool leaf_single, hipStream_t st);
void launch_service_any_device(const DevScene& sc, const ServiceRays& r, uint8_t* occluded, uint32_t* invalid, const TraceWorkspace& ws, unsigned long long* gstats,
							   hipStream_t st);
void launch_service_geometry(const DevScene& sc, const ServiceRays& r, const ServiceHits& h, hipStream_t st); // GeomPoint of every ray that hit, zeros / INVALID for the others
// What prgpu_enable_ambient_occlusion allocates; passed by value.
struct AoState {
	float4* rec;			// 4 per hit: (P, slot bits), (N, state low), (Nx, state high), (Ny, 0)
	uint32_t* occluded;		// per hit: occluded rays of this iteration
	const uint64_t* jump;	// PCG_MULT^(2 k), k < sample_count
	uint32_t* counts;		// per pixel: occluded rays over all iterations (prgpu_download_ao_counts)
	uint64_t jump_all;		// PCG_MULT^(2 sample_count)
	uint32_t sample_count;
	// debug record of the last iteration (instrumented kernels only; cleared before every iteration): per pixel the generator state, per pixel and sample the ray
	uint64_t* dbg_state;
	float* dbg_org;
	float* dbg_dir;
	uint8_t* dbg_occluded;
};

// Ambient occlusion pipeline (device/ao.inl): the three passes between k_trace_closest and k_resolve of an iteration.  `n_hits` is the device
// counter the closest-hit launch zeroes (its shade_counters[0]); no pass needs it on the host.  instrumented: traversal counters + ray dump.
void launch_ao_hits(const DevScene& sc, const PathState& ps, const AoState& ao, uint32_t n_slots, bool instrumented, uint32_t* n_hits, uint32_t* queue_head_closest,
					uint32_t* queue_head_ao, unsigned long long* gstats, hipStream_t st);
void launch_ao_occlusion(const DevScene& sc, const PathState& ps, const AoState& ao, uint32_t n_slots, bool instrumented, const uint32_t* n_hits, const TraceWorkspace& ws,
						 unsigned long long* gstats, hipStream_t st);
void launch_ao_splat(const DevScene& sc, const PathState& ps, const AoState& ao, uint32_t n_slots, const uint32_t* n_hits, hipStream_t st);
bool ao_counts_folded(); // how the occlusion kernel was built (PR_AO_FOLD): one atomic per hit and wave step, or one per occluded ray

// Visual feedback pipeline (device/vf.inl): ONE pass between k_trace_closest and k_resolve of an iteration.
// Rows of the colour table (tables/pr_vf_colors.inl): the 23 colours an id selects by id % 23, then green (= True), red (= False), blue.
constexpr uint32_t VF_RANDOM_COLOURS = 23, VF_GREEN = 23, VF_RED = 24, VF_BLUE = 25, VF_COLOURS = 26;
// What prgpu_enable_visual_feedback sets up; passed by value.
struct VfState {
	const float4* colours; // VF_COLOURS rows: the upsampler's three coefficients of the colour (prgpu_rgb_to_coeffs), w unused
	uint32_t mode;		   // PRGPU_VF_*
	uint32_t weighting;	   // radiance *= |NdotV| (every mode but PRGPU_VF_NDOTV)
};
void launch_vf_shade(const DevScene& sc, const PathState& ps, const VfState& vf, uint32_t n_slots, uint32_t* queue_head_closest, unsigned long long* gstats, hipStream_t st);
} // namespace prd
