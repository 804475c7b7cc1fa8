// libspath_hip.so -- C ABI (include/spath_hip.h) over the gfx950 kernels in sp_kernels.h.
//
// Host side of the drop-in boundary: owns the device buffers (grow-only, like the reference's
// OpenCL peer caches its cl::Buffers, src/cl_renderer.cpp:107-112), uploads what
// renderer::render / render_flat are handed (src/renderer.h:31-32), launches, reads back.
// No exception crosses this boundary; every failure becomes a status + sphip_last_error().
#include "spath_hip.h"
#include "sp_kernels.h"
#include "sp_cyl_scan.h"
#include "sp_scan_kernels.h"
#include "sp_bvh.h"
#include "sp_bvh_build.h"
#include "sp_adaptive.h"
#include "sp_denoise.h"
#include "sp_reproject.h"
#include "sp_display.h"
#include "sp_environment.h"
#include "sp_host_plan.h"
#include "sp_host_tables.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdlib>
#include <dlfcn.h>
#include <thread>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace {
using namespace sp_host;       // the launch plan, the light tables, the rules of the per-triangle tables: what needs no device (sp_host_*.h)

thread_local std::string g_create_error;

struct DevBuf {
	void* p = nullptr;
	size_t cap = 0;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;                // owns p: freed with the context (sphip_destroy makes its device current first)
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { if (p) (void)hipFree(p); }
};

} // namespace

struct sphip_ctx {
	int device = 0;
	hipStream_t own_stream = nullptr;       // host-pointer path
	hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr, ev_u0 = nullptr, ev_u1 = nullptr, ev_d0 = nullptr, ev_d1 = nullptr;
	DevBuf tris, mats, scan, bounds, samp, rays, rgba, accum, counter, work, bvh_nodes, bvh_rec, bvh_idx, sort_kv, sort_hist, bvh_meta, cyl_rec, cyl_cnt, cyl_hdr, prim, cylm_rec, cylm_hdr, cylm_big;
	// record streams beyond the exact one are derived from `tris` the first time a kernel variant that reads them runs on the scene
	bool bvh_valid = false, cyl_valid = false, cylm_valid = false;
	bool cylm_wide = false;                 // the stream in cylm_rec is laid out for the 512-thread shape of the default scan (sp_cylm_both.h)
	uint32_t bvh_leaves = 0;
	size_t n_tris = 0;
	bool have_scene = false;
	bool have_render = false, timed_upload = false, timed_download = false;
	sphip_stats stats{};
	std::string err;
	std::string desc;
	hipStream_t last_stream = nullptr;
	// ---- multi-device context (sphip_create_multi): one child context per listed device; the exchange buffers live on the
	// first child's device.  A single-device context has no kids.
	std::vector<sphip_ctx*> kids;
	int gather_kind = SPHIP_GATHER_NONE;
	void* rccl_lib = nullptr;
	std::vector<void*> comms;                     // ncclComm_t per child
	DevBuf gath, gath_acc, img, img_acc;           // [n_dev][pad] tiles as gathered, and the image in pixel order
	std::vector<hipEvent_t> ev_tile;               // child r's tiles have arrived on the first device
	hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;
	// ---- progressive accumulation (sphip_accum_begin / sphip_accum_step).  The rays and the running sum of the frame (of this
	// device's shard, on a child of a multi-device context) live in buffers of their own, so that renders issued between two
	// steps do not disturb them; the parameters are the parent's.
	DevBuf acc_rays, acc_sum;
	bool acc_on = false;                          // an accumulation has been begun
	bool acc_stale = false;                       // ... and a scene has been set since
	size_t acc_w = 0, acc_h = 0;
	uint64_t acc_seed = 0, acc_total = 0;         // acc_total: samples accumulated so far
	int acc_flags = 0;
	// ---- adaptive sampling (sphip_accum_begin_adaptive) on top of that accumulation; per local pixel: S1/S2 (16 B), the sample
	// count, two active lists (the step's and the next), the active rays gathered in list order, a keep byte; per 256 pixels one
	// block total.  adp_nact: pixels still active (host copy, read back with each step's image); on a multi-device context the
	// sum over the devices, the rule being the parent's
	DevBuf adp_s12, adp_cnt, adp_list[2], adp_rays, adp_keep, adp_blk, adp_nact_d, adp_wst;
	bool adp_on = false;
	int adp_cur = 0;                              // adp_list[adp_cur] is the current list
	uint32_t adp_nact = 0, adp_nact_rb = 0;       // adp_nact_rb: the step's readback, valid once the stream has drained
	double adp_t = 0.0, adp_floor = 0.0;
	uint32_t adp_min = 0;
	// ---- denoising (sp_denoise.h): material classes of the scene's triangles (derived on first use), the closest hits of a
	// G-buffer build, the accumulation's cached G-buffer, the filter's ping-pong buffers.  On a multi-device context the parent's
	// buffers live on the first device, with the whole frame's rays gathered there for the G-buffer.
	DevBuf dn_cls, dn_hit, dn_gbuf, dn_a, dn_b, dn_rays;
	bool dn_cls_valid = false;                    // dropped by every set_scene
	// ---- next-event estimation (SPHIP_FLAG_NEE): the scene's light table (sp_host_plan.h: LightTable, laid out by pack_light_table), built on
	// the host from a read-back on the first NEE render after a scene change; nee_bad: the scene has an invalid emittance (nee_msg says which)
	DevBuf nee_tab;
	bool nee_valid = false, nee_bad = false;      // nee_valid dropped by every set_scene
	uint32_t nee_n = 0;
	double nee_W = 0.0;
	std::string nee_msg;
	bool dn_gbuf_ok = false;                      // dropped by every accumulation begin
	// ---- camera samples (SPHIP_FLAG_CAMERA_SAMPLES): the lens of later renders (sphip_set_lens; the parent's on a multi-device context),
	// and what an accumulation begun with a camera captured: the camera and the lens of its begin
	sphip_lens lens{};
	sphip_lens acc_lens{};
	sphip_camera acc_cam{};
	bool acc_has_cam = false;
	// ---- temporal reprojection (sp_reproject.h, sphip_accum_reproject): the history attached to the current accumulation (the reprojected
	// mean and count per pixel), and what a reprojection reads of the view it leaves: its rays, G-buffer, blended mean and count
	// (rp_pmean doubles as the blended mean sphip_accum_denoise filters).  Every one is written whole before it is read.
	DevBuf rp_hmean, rp_hist, rp_prays, rp_pgbuf, rp_pmean, rp_phist;
	bool acc_hist_on = false;                     // dropped by every accumulation begin
	// ---- display transform (sp_display.h, sphip_accum_display): the luminance histogram of a metered call and the display-linear float
	// output; scratch of one call, nothing another call reads
	DevBuf dp_hist, dp_rgb;
	// ---- the per-triangle tables of the scene (sp_host_tables.h: kTriTables; kTableSlots below names each one's members).  One rule for
	// all: a table belongs to the scene last set and is kept like it, so every set_scene drops it (drop_tables); every device of a
	// multi-device context keeps the whole table; a render reads it while its flag is set.  What is particular to each:
	//   spec   SPHIP_FLAG_SPECULAR    4 floats per triangle
	//   vnorm  SPHIP_FLAG_SMOOTH      9 floats per triangle
	//   glass  SPHIP_FLAG_DIELECTRIC  4 floats per triangle; setting it allocates spec_zero (ensure_zero_rows)
	//   rough  SPHIP_FLAG_GLOSSY      1 float per triangle
	//   uv     SPHIP_FLAG_TEXTURE     6 floats per triangle; rendered with the context's atlas (below)
	DevBuf spec, vnorm, glass, rough, uv;
	bool have_spec = false, have_vnorm = false, have_glass = false, have_rough = false, have_uv = false;
	// what stands in for a table or a map whose flag is off: spec_zero, a float4 of zeros for each of the scene's first zero_rows triangles
	// (the specular table of a dielectric render, either table of an environment render, the roughness table of a textured one), and
	// env_black, the 1 x 1 black map (texel, rc, marg and tpdf all zeros, T = 0) of a glossy render without SPHIP_FLAG_ENVIRONMENT: it adds
	// no entry to the light table and every miss carries 0
	DevBuf spec_zero, env_black;
	size_t zero_rows = 0;
	// ---- environment lighting (sp_environment.h): the octahedral map env_n x env_n x 3 f32 and its importance tables wt, rc, marg (double),
	// built on the device by both setters; every device of a multi-device context keeps them.  NOT dropped by set_scene: the map does not
	// depend on the triangles.  What does (env_T read back, w_env, W and tpdf: ensure_env_lights) is rebuilt on first use after either changes
	DevBuf env_tex, env_wt, env_rc, env_marg, env_tpdf;
	bool have_env = false, env_lights_valid = false;
	uint32_t env_n = 0;
	double env_T = 0.0, env_wenv = 0.0, env_W = 0.0;
	// SPHIP_FLAG_ENVIRONMENT: the flagged light table (the triangle entries under the total W that includes w_env, then the map's entry;
	// laid out like nee_tab), built by ensure_env_lights from the host copy of the unflagged one; without an entry it is nee_tab itself.
	// env_M: where the two-stage kernels park the miss term
	DevBuf env_tab, env_M;
	uint32_t env_nee_n = 0;
	sp_host::LightTable nee_host;                  // the host copy of nee_tab: what the flagged table is made from
	// ---- textures (SPHIP_FLAG_TEXTURE): the atlas tex_w x tex_h x 3 f32, context-level like the environment map: NOT dropped by
	// set_scene; every device of a multi-device context keeps it.  tex_A: where the two-stage kernels park the albedo per depth
	DevBuf atlas, tex_A;
	bool have_tex = false;
	uint32_t tex_w = 0, tex_h = 0;
	// ---- normal mapping (SPHIP_FLAG_NORMAL_MAP): the map nmap_w x nmap_h x 3 f32 (signed tangent-space vectors), kept like the atlas.  What
	// stands in when SPHIP_FLAG_SMOOTH or SPHIP_FLAG_TEXTURE is off: vnorm_zero, 9 floats of zeros for each of the scene's first
	// vnorm_zero_rows triangles (every triangle flat), and tex_white, the 1 x 1 white atlas (rho * 1.0f = rho)
	DevBuf nmap, vnorm_zero, tex_white;
	bool have_nmap = false;
	uint32_t nmap_w = 0, nmap_h = 0;
	size_t vnorm_zero_rows = 0;
};

namespace {

int fail(sphip_ctx* c, int code, const char* fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	if (c) c->err = buf; else g_create_error = buf;
	return code;
}

#define HIP_TRY(c, expr)                                                                         \
	do {                                                                                         \
		hipError_t e_ = (expr);                                                                  \
		if (e_ != hipSuccess)                                                                    \
			return fail((c), SPHIP_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
	} while (0)

// where table k of kTriTables lives in a context
struct TableSlot { DevBuf sphip_ctx::*buf; bool sphip_ctx::*have; };
const TableSlot kTableSlots[kTriTableCount] = {
	{ &sphip_ctx::spec, &sphip_ctx::have_spec }, { &sphip_ctx::vnorm, &sphip_ctx::have_vnorm }, { &sphip_ctx::glass, &sphip_ctx::have_glass },
	{ &sphip_ctx::rough, &sphip_ctx::have_rough }, { &sphip_ctx::uv, &sphip_ctx::have_uv },
};
static_assert(kTriTables[kTabSpecular].max_tris == (size_t)sp::kSpecBit && kTriTables[kTabDielectric].max_tris == (size_t)sp::kTransBit,
              "the triangle limits of sp_host_tables.h are the path history's marker bits");
// every table belongs to the scene that is being replaced
void drop_tables(sphip_ctx* c) { for (const TableSlot& s : kTableSlots) c->*s.have = false; }

// the guard of the device-pointer entry points: a context, and a single-device one
int single_device_entry(sphip_ctx* c) {
	if (!c) return SPHIP_E_INVALID;
	return c->kids.empty() ? SPHIP_OK : fail(c, SPHIP_E_STATE, "device-pointer entry points need a single-device context (sphip_create)");
}

int ensure(sphip_ctx* c, DevBuf& b, size_t bytes) {
	if (bytes <= b.cap && b.p) return SPHIP_OK;
	if (b.p) { HIP_TRY(c, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
	const size_t want = bytes < 256 ? 256 : bytes;
	HIP_TRY(c, hipMalloc(&b.p, want));
	b.cap = want;
	return SPHIP_OK;
}

// kernel variants selectable through the low byte of `flags` (sphip_kernel_name); all brute force except 8
constexpr int kVariantAccel = 8;          // the opt-in acceleration structure (SPHIP_FLAG_ACCEL)
constexpr int kVariantLast = 16;
// One row per variant number, with its TwoStage shape (sp_host_plan.h; scan 3, the default, gets its 512-thread shape 4 from plan_render).
// The library carries the exact-only scans (1, 2), the opt-in BVH (8), one f32 cylinder scan for A/B runs (15) and the default (16).  The
// slab-filter scans (3-7) and the earlier cylinder scans (9-14) are retired: their numbers keep their names (sphip_kernel_name) and are refused.
struct Variant { const char* name; TwoStage ts; bool carried; };
const Variant kVariants[kVariantLast + 1] = {
	{ "auto",         {0, false, 0}, false },
	{ "rpl_sload",    {0, false, 0}, true  },
	{ "rpl_lds",      {0, false, 0}, true  },
	{ "rpl_filter2",  {2, false, 0}, false },
	{ "rpl_filter4",  {4, false, 0}, false },
	{ "rpl_filter1",  {1, false, 0}, false },
	{ "rpl_filter2s", {2, true,  0}, false },
	{ "rpl_filter4s", {4, true,  0}, false },
	{ "accel_lbvh",   {0, false, 0}, true  },
	{ "rpl_cyl1",     {1, false, 1}, false },
	{ "rpl_cyl2",     {2, false, 1}, false },
	{ "rpl_cyl4",     {4, false, 1}, false },
	{ "rpl_cyl2s",    {2, true,  1}, false },
	{ "rpl_cyl4s",    {4, true,  1}, false },
	{ "rpl_cylw4",    {4, false, 2}, false },
	{ "rpl_cylw4s",   {4, true,  2}, true  },
	{ "rpl_cylm",     {1, false, 3}, true  },
};
bool variant_carried(int v) { return v >= 1 && v <= kVariantLast && kVariants[v].carried; }
// smooth shading is built for the exact scan, the BVH and the default scan (both shapes)
bool variant_smooth(int v) { return v == 1 || v == kVariantAccel || v == 16; }

int pick_variant(int flags, size_t n_tris) {
	if (flags & SPHIP_FLAG_ACCEL) return kVariantAccel;
	const int v = flags & SPHIP_KERNEL_MASK;
	if (v >= 1 && v <= kVariantLast) return v;
	if (n_tris < 64) return 1;        // tiny scenes: nothing to filter, the scalar path has no barriers
	if (n_tris >= (1ull << sp::kMIdxBits)) return 15;      // the default scan packs (ray, triangle index) into 32 bits: 6 + 26
	// The third-generation scan (sp_cylm_scan.h: stage 1 on the f16 matrix pipe, one ray per lane) for every mode; sample chunks
	// (plan_launch) supply the workgroups a small frame lacks.
	return 16;
}

// exact records + scene bound: what every variant reads.  The other streams are built on first use (ensure_* below).
int repack(sphip_ctx* c, hipStream_t st) {
	const uint32_t n = (uint32_t)c->n_tris;
	const uint32_t n_pad = (n / sp::kTile + 1) * sp::kTile;      // whole LDS tiles and at least one zero record behind n (index n: the padding of the two-stage streams points at it)
	int rc;
	if ((rc = ensure(c, c->scan, (size_t)n_pad * 48)) || (rc = ensure(c, c->bounds, 256))) return rc;
	HIP_TRY(c, hipMemsetAsync(c->bounds.p, 0, 256, st));
	hipLaunchKernelGGL(sp::k_repack, dim3((n_pad + 255) / 256), dim3(256), 0, st,
	                   (const float*)c->tris.p, (float4*)c->scan.p, (unsigned int*)c->bounds.p, n, n_pad);
	HIP_TRY(c, hipGetLastError());
	c->have_scene = true;
	c->bvh_valid = c->cyl_valid = c->cylm_valid = false;
	c->nee_valid = false;
	c->env_lights_valid = false;                   // w_env and tpdf follow the scene; the map itself stays
	c->zero_rows = 0;
	drop_tables(c);
	return SPHIP_OK;
}

// stable radix sort of n (key, value) pairs held in c->sort_kv as keys[2][n], vals[2][n] (sp_radix_sort.h); returns which half holds the result
int radix_sort(sphip_ctx* c, uint32_t n, uint32_t key_bits, hipStream_t st, int* out_half) {
	const uint32_t rs_blocks = (n + sp::kRsPerBlock - 1) / sp::kRsPerBlock;
	int rc = ensure(c, c->sort_hist, (size_t)rs_blocks * 16 * 4);
	if (rc) return rc;
	uint32_t* keys[2] = { (uint32_t*)c->sort_kv.p, (uint32_t*)c->sort_kv.p + (size_t)n };
	uint32_t* vals[2] = { (uint32_t*)c->sort_kv.p + (size_t)2 * n, (uint32_t*)c->sort_kv.p + (size_t)3 * n };
	int cur = 0;
	for (uint32_t shift = 0; shift < key_bits; shift += 4, cur ^= 1) {
		hipLaunchKernelGGL(sp::k_rs_hist, dim3(rs_blocks), dim3(256), 0, st, (const uint32_t*)keys[cur], n, shift, rs_blocks, (uint32_t*)c->sort_hist.p);
		hipLaunchKernelGGL(sp::k_rs_scan, dim3(1), dim3(256), 0, st, (uint32_t*)c->sort_hist.p, rs_blocks * 16u);
		hipLaunchKernelGGL(sp::k_rs_scatter, dim3(rs_blocks), dim3(256), 0, st, (const uint32_t*)keys[cur], (const uint32_t*)vals[cur], n, shift, rs_blocks,
		                   (const uint32_t*)c->sort_hist.p, keys[cur ^ 1], vals[cur ^ 1]);
	}
	HIP_TRY(c, hipGetLastError());
	*out_half = cur;
	return SPHIP_OK;
}

// ---- the default scan's stream (sp_cylm_scan.h): classes by dominant axis, ascending cylinder radius within a class (device sort),
// tiles of kMTile triangles: f32 records + f16 matrix fragments + the per-group Hmax table
template <bool WIDE>
int build_cylm(sphip_ctx* c, hipStream_t st) {
#define SP_CM(x) (WIDE ? sp::cylm512::x : sp::cylm256::x)
	const uint32_t n = (uint32_t)c->n_tris, nblocks = (n + 255) / 256, max_tiles = n / SP_CM(kMTile) + 4;
	int rc;
	if ((rc = ensure(c, c->sort_kv, (size_t)n * 16)) || (rc = ensure(c, c->cylm_hdr, 256)) || (rc = ensure(c, c->cylm_big, sp::cylm256::kMBig * 48)) ||
	    (rc = ensure(c, c->cylm_rec, (size_t)max_tiles * SP_CM(kMTileQ) * 16))) return rc;
	uint32_t* keys = (uint32_t*)c->sort_kv.p;
	uint32_t* vals = (uint32_t*)c->sort_kv.p + (size_t)2 * n;
	uint32_t* hdr = (uint32_t*)c->cylm_hdr.p;
	const float* tris = (const float*)c->tris.p;
	const unsigned int* bnd = (const unsigned int*)c->bounds.p;
	float4* rec = (float4*)c->cylm_rec.p;
	HIP_TRY(c, hipMemsetAsync(hdr, 0, 256, st));
	// (the class, key and big-class kernels do not depend on the tile size)
	hipLaunchKernelGGL(sp::cylm256::k_cylm_count_big, dim3(nblocks), dim3(256), 0, st, tris, n, bnd, hdr);
	hipLaunchKernelGGL(sp::cylm256::k_cylm_keys, dim3(nblocks), dim3(256), 0, st, tris, n, bnd, keys, vals, hdr);
	int half = 0;
	if ((rc = radix_sort(c, n, 32, st, &half))) return rc;
	const uint32_t* sorted = vals + (size_t)half * n;
	hipLaunchKernelGGL(SP_CM(k_cylm_hdr), dim3(1), dim3(1), 0, st, hdr, bnd);
	hipLaunchKernelGGL(SP_CM(k_cylm_scatter), dim3(nblocks), dim3(256), 0, st, tris, n, sorted, (const uint32_t*)hdr, rec, (const float4*)c->scan.p, (float4*)c->cylm_big.p);
	hipLaunchKernelGGL(SP_CM(k_cylm_pad), dim3(3), dim3(256), 0, st, (const uint32_t*)hdr, n, rec);
	hipLaunchKernelGGL(SP_CM(k_cylm_hmax), dim3(max_tiles), dim3(SP_CM(kMGroups)), 0, st, tris, n, (const uint32_t*)hdr, rec);
#undef SP_CM
	HIP_TRY(c, hipGetLastError());
	c->cylm_valid = true;
	c->cylm_wide = WIDE;
	return SPHIP_OK;
}

// which shape of the default scan serves this scene (SPATH_HIP_CYLM_SHAPE=256|512 overrides, for A/B runs)
bool cylm_wants_wide(const sphip_ctx* c) {
	if (const char* e = getenv("SPATH_HIP_CYLM_SHAPE")) return atoi(e) == 512;
	return c->n_tris >= sp::kMBigSceneTris;
}

int ensure_cylm(sphip_ctx* c, hipStream_t st) {
	if (c->cylm_valid) return SPHIP_OK;
	return cylm_wants_wide(c) ? build_cylm<true>(c, st) : build_cylm<false>(c, st);
}

// ---- class-sorted f32 cylinder records (sp_cyl_scan.h): count per block -> offsets -> scatter -> pad, all on the device
int ensure_cyl(sphip_ctx* c, hipStream_t st) {
	if (c->cyl_valid) return SPHIP_OK;
	const uint32_t n = (uint32_t)c->n_tris, nblocks = (n + 255) / 256;
	int rc;
	if ((rc = ensure(c, c->cyl_cnt, (size_t)nblocks * 3 * sizeof(uint32_t))) || (rc = ensure(c, c->cyl_hdr, 256)) ||
	    (rc = ensure(c, c->cyl_rec, ((size_t)n / sp::kCylTile + 4) * sp::kCylTile * 32))) return rc;
	hipLaunchKernelGGL(sp::k_cyl_count, dim3(nblocks), dim3(256), 0, st, (const float*)c->tris.p, n, (uint32_t*)c->cyl_cnt.p);
	hipLaunchKernelGGL(sp::k_cyl_offsets, dim3(1), dim3(256), 0, st, (uint32_t*)c->cyl_cnt.p, nblocks, (uint32_t*)c->cyl_hdr.p, sp::kCylTile);
	hipLaunchKernelGGL(sp::k_cyl_scatter, dim3(nblocks), dim3(256), 0, st, (const float*)c->tris.p, n, (const uint32_t*)c->cyl_cnt.p,
	                   (const uint32_t*)c->cyl_hdr.p, (float4*)c->cyl_rec.p);
	hipLaunchKernelGGL(sp::k_cyl_pad, dim3(3), dim3(256), 0, st, (const uint32_t*)c->cyl_hdr.p, n, (float4*)c->cyl_rec.p);
	HIP_TRY(c, hipGetLastError());
	c->cyl_valid = true;
	return SPHIP_OK;
}

// ---- linear BVH for SPHIP_FLAG_ACCEL (sp_bvh.h), built on the device (sp_bvh_build.h) the first time a scene is rendered with the flag
int ensure_bvh(sphip_ctx* c, hipStream_t st) {
	if (c->bvh_valid) return SPHIP_OK;
	const uint32_t n = (uint32_t)c->n_tris;
	uint32_t nl = 1;
	while ((uint64_t)nl * 4 < n) nl <<= 1;                 // leaves of 4 triangles, padded to a power of two (complete tree in heap order)
	const uint32_t nblocks = (n + 255) / 256;
	int rc;
	if ((rc = ensure(c, c->bvh_nodes, (size_t)2 * nl * 32)) || (rc = ensure(c, c->bvh_rec, ((size_t)nl * 4 + sp::kBvhMaxBig) * 48)) ||
	    (rc = ensure(c, c->bvh_idx, ((size_t)nl * 4 + sp::kBvhMaxBig) * 4)) || (rc = ensure(c, c->sort_kv, (size_t)n * 16)) ||
	    (rc = ensure(c, c->bvh_meta, 256))) return rc;
	uint32_t* meta = (uint32_t*)c->bvh_meta.p;
	uint32_t* vals[2] = { (uint32_t*)c->sort_kv.p + (size_t)2 * n, (uint32_t*)c->sort_kv.p + (size_t)3 * n };
	const float* tris = (const float*)c->tris.p;
	const dim3 b256(256);
	hipLaunchKernelGGL(sp::k_bvh_meta_init, dim3(1), b256, 0, st, meta);
	hipLaunchKernelGGL(sp::k_bvh_box, dim3(nblocks), b256, 0, st, tris, n, meta);
	hipLaunchKernelGGL(sp::k_bvh_count_big, dim3(nblocks), b256, 0, st, tris, n, meta);
	hipLaunchKernelGGL(sp::k_bvh_keys, dim3(nblocks), b256, 0, st, tris, n, meta, (uint32_t*)c->sort_kv.p, vals[0]);
	int cur = 0;
	if ((rc = radix_sort(c, n, 32, st, &cur))) return rc;            // stable LSD radix sort by (Morton code; big triangles last)
	hipLaunchKernelGGL(sp::k_bvh_leaves, dim3((nl + 255) / 256), b256, 0, st, tris, n, (const uint32_t*)meta, (const uint32_t*)vals[cur], nl,
	                   (float4*)c->bvh_nodes.p, (float4*)c->bvh_rec.p, (int*)c->bvh_idx.p);
	hipLaunchKernelGGL(sp::k_bvh_bigs, dim3(1), b256, 0, st, tris, n, (const uint32_t*)meta, (const uint32_t*)vals[cur], nl, (float4*)c->bvh_rec.p, (int*)c->bvh_idx.p);
	for (uint32_t first = nl >> 1; first >= 1; first >>= 1)              // bottom-up, one level per launch
		hipLaunchKernelGGL(sp::k_bvh_refit, dim3((first + 255) / 256), b256, 0, st, (float4*)c->bvh_nodes.p, first);
	HIP_TRY(c, hipGetLastError());
	c->bvh_leaves = nl;
	c->bvh_valid = true;
	return SPHIP_OK;
}

// a light table (sp_host_plan.h) into device buffer b, which keeps 16 spare bytes so that a table without entries has a buffer too
int upload_light_table(sphip_ctx* c, DevBuf& b, const LightTable& t, hipStream_t st) {
	const std::vector<char> blob = pack_light_table(t);
	if (const int rc = ensure(c, b, blob.size() + 16)) return rc;
	if (blob.empty()) return SPHIP_OK;
	HIP_TRY(c, hipMemcpyAsync(b.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipStreamSynchronize(st));             // blob is a local
	return SPHIP_OK;
}

// ---- the light table of next-event estimation (build_light_table), from a read-back on the first NEE render after a scene change
int ensure_lights(sphip_ctx* c, hipStream_t st) {
	if (c->nee_valid) return c->nee_bad ? fail(c, SPHIP_E_INVALID, "%s", c->nee_msg.c_str()) : SPHIP_OK;
	const size_t n = c->n_tris;
	std::vector<float> t(n * 12), m(n * 6);
	HIP_TRY(c, hipMemcpyAsync(t.data(), c->tris.p, n * 48, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(m.data(), c->mats.p, n * 24, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	LightTable lt = build_light_table(t.data(), m.data(), n);
	c->nee_bad = lt.bad_tri != SIZE_MAX;
	if (c->nee_bad) {
		char buf[160];
		snprintf(buf, sizeof buf, "SPHIP_FLAG_NEE: triangle %zu has emittance component %d = %g (must be finite and >= 0)", lt.bad_tri, lt.bad_comp,
		         (double)m[lt.bad_tri * 6 + 3 + lt.bad_comp]);
		c->nee_msg = buf;
		c->nee_valid = true;
		return fail(c, SPHIP_E_INVALID, "%s", buf);
	}
	if (const int rc = upload_light_table(c, c->nee_tab, lt, st)) return rc;
	c->nee_n = (uint32_t)lt.cdf.size();
	c->nee_W = lt.W;
	c->nee_host = std::move(lt);
	c->nee_valid = true;
	return SPHIP_OK;
}

// ---- environment lighting (include/spath_hip.h "environment lighting").  The map's own tables, on the stream
// that carries the texels: wt per texel, rc one thread per row, marg one thread (the order of the double additions is the contract)
int build_env_tables(sphip_ctx* c, uint32_t n, hipStream_t st) {
	const size_t nn = (size_t)n * n;
	int rc;
	if ((rc = ensure(c, c->env_wt, nn * 8)) || (rc = ensure(c, c->env_rc, nn * 8)) || (rc = ensure(c, c->env_marg, (size_t)n * 8)) || (rc = ensure(c, c->env_tpdf, nn * 4))) return rc;
	hipLaunchKernelGGL(sp::k_env_wt, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, (const float*)c->env_tex.p, n, (double*)c->env_wt.p);
	hipLaunchKernelGGL(sp::k_env_rows, dim3((n + 255u) / 256u), dim3(256), 0, st, (const double*)c->env_wt.p, n, (double*)c->env_rc.p);
	hipLaunchKernelGGL(sp::k_env_marg, dim3(1), dim3(64), 0, st, (const double*)c->env_rc.p, n, (double*)c->env_marg.p);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipMemsetAsync(c->env_tpdf.p, 0, nn * 4, st));       // no light table yet: the map is not sampled
	return SPHIP_OK;
}

// the map of a single-device context from src (n * n * 3 f32), or no map with src == nullptr; sync: src is borrowed host memory
int set_env_map(sphip_ctx* c, const void* src, uint32_t n, hipMemcpyKind kind, hipStream_t st, bool sync) {
	c->acc_stale = c->acc_on;                      // the running sum was rendered under the old map
	c->have_env = false;
	c->env_lights_valid = false;
	if (!src) return SPHIP_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	const size_t bytes = (size_t)n * n * 12;
	int rc;
	if ((rc = ensure(c, c->env_tex, bytes))) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->env_tex.p, src, bytes, kind, st));
	if ((rc = build_env_tables(c, n, st))) return rc;
	if (sync) HIP_TRY(c, hipStreamSynchronize(st));
	c->env_n = n;
	c->have_env = true;
	return SPHIP_OK;
}

// the scene-dependent part, on first use after the map or the scene changed: T = marg[n - 1] read back, Phi = T * (4 / (n n)),
// w_env = 0.5 * R2 * Phi with R2 a quarter of the squared diagonal of the scene's bounding box (the power through the scene's bounding
// disc, in the light table's units A * Esum), W = the triangle table's total + w_env, and tpdf.  !(T > 0): no entry, W is the triangles'
int ensure_env_lights(sphip_ctx* c, hipStream_t st) {
	if (c->env_lights_valid) return SPHIP_OK;
	int rc;
	if ((rc = ensure_lights(c, st))) return rc;
	const size_t nt = c->n_tris;
	const uint32_t n = c->env_n;
	std::vector<float> t(nt * 12);
	double T = 0.0;
	HIP_TRY(c, hipMemcpyAsync(t.data(), c->tris.p, nt * 48, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(&T, (const double*)c->env_marg.p + (n - 1u), 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	float lo[3] = { t[0], t[1], t[2] }, hi[3] = { t[0], t[1], t[2] };
	for (size_t i = 0; i < nt; ++i)
		for (int v = 0; v < 3; ++v)
			for (int k = 0; k < 3; ++k) {
				const float x = t[i * 12 + 3 * v + k];
				if (x < lo[k]) lo[k] = x;
				if (x > hi[k]) hi[k] = x;
			}
	const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
	const double R2 = 0.25 * ((dx * dx + dy * dy) + dz * dz);
	const double Phi = T * (4.0 / ((double)n * (double)n));
	const double w_env = T > 0.0 ? (0.5 * R2) * Phi : 0.0;
	const bool entry = w_env > 0.0;                // a black map, or a scene whose bounding box is a point: no entry
	c->env_T = T;
	c->env_wenv = entry ? w_env : 0.0;
	c->env_W = entry ? c->nee_W + c->env_wenv : c->nee_W;
	const double sel = entry ? c->env_wenv / c->env_W : 0.0;
	const size_t nn = (size_t)n * n;
	hipLaunchKernelGGL(sp::k_env_tpdf, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, (const double*)c->env_wt.p, n, sel, T, (float*)c->env_tpdf.p);
	HIP_TRY(c, hipGetLastError());
	// the flagged light table (flagged_light_table).  A black map adds nothing: the render then reads the unflagged table, bit for bit
	c->env_nee_n = c->nee_n;
	if (entry) {
		const LightTable ft = flagged_light_table(c->nee_host, c->env_W, nt);
		if ((rc = upload_light_table(c, c->env_tab, ft, st))) return rc;
		c->env_nee_n = (uint32_t)ft.cdf.size();
	}
	c->env_lights_valid = true;
	return SPHIP_OK;
}

// the zeros that stand in for a per-triangle table whose flag is off (the specular table of a dielectric render, either table of an
// environment render, the roughness table of a textured one: its first float per triangle): one float4 row per triangle of the scene.  put_table calls this before it makes the device current
int ensure_zero_rows(sphip_ctx* c, hipStream_t st) {
	if (c->zero_rows == c->n_tris) return SPHIP_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	if (const int rc = ensure(c, c->spec_zero, c->n_tris * 16)) return rc;
	HIP_TRY(c, hipMemsetAsync(c->spec_zero.p, 0, c->n_tris * 16, st));
	c->zero_rows = c->n_tris;
	return SPHIP_OK;
}

// the 1 x 1 black map of a glossy render without SPHIP_FLAG_ENVIRONMENT: zeros, written once per context
int ensure_black_map(sphip_ctx* c, hipStream_t st) {
	if (c->env_black.p) return SPHIP_OK;
	if (const int rc = ensure(c, c->env_black, 256)) return rc;
	HIP_TRY(c, hipMemsetAsync(c->env_black.p, 0, 256, st));
	HIP_TRY(c, hipStreamSynchronize(st));          // later renders may come on another stream
	return SPHIP_OK;
}

// the stand-ins of a normal-mapped render (sphip_ctx): the zero vertex normals of the scene's triangles ...
int ensure_zero_vnorm(sphip_ctx* c, hipStream_t st) {
	if (c->vnorm_zero_rows == c->n_tris && c->vnorm_zero.p) return SPHIP_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	if (const int rc = ensure(c, c->vnorm_zero, c->n_tris * 36)) return rc;
	HIP_TRY(c, hipMemsetAsync(c->vnorm_zero.p, 0, c->n_tris * 36, st));
	HIP_TRY(c, hipStreamSynchronize(st));          // later renders may come on another stream; once per scene
	c->vnorm_zero_rows = c->n_tris;
	return SPHIP_OK;
}
// ... and the 1 x 1 white atlas, written once per context
int ensure_white_texel(sphip_ctx* c, hipStream_t st) {
	if (c->tex_white.p) return SPHIP_OK;
	static const float one[3] = { 1.0f, 1.0f, 1.0f };
	if (const int rc = ensure(c, c->tex_white, 256)) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->tex_white.p, one, sizeof one, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipStreamSynchronize(st));          // later renders may come on another stream
	return SPHIP_OK;
}

constexpr int kModeHits = 2;   // internal: sphip_closest_hit_device

// f(args...) with the trailing pack of a path-tracing kernel for the run-time choices, always in the kernels' order: the running
// sum (nothing, AccumArgs or AdaptArgs), the estimator (nothing, NeeArgs or MisArgs), the specular table (nothing or SpecArgs), the
// vertex normals (nothing or NormArgs), the camera (nothing or CamArgs).  Each combination is a kernel of its own; the two tables
// are composed with the plain estimator and with MIS only (launch_render rejects them with NEE alone), and f prunes the other ones
// that are not built with if constexpr on the pack traits (sp_kernels.h).
template <typename F>
void with_accum(const sp::AccumArgs* prog, const sp::AdaptArgs* ad, F&& f) {
	if (ad) f(*ad);
	else if (prog) f(*prog);
	else f();
}
template <typename F>
void with_pack(const sp::AccumArgs* prog, const sp::AdaptArgs* ad, const sp::NeeArgs* ne, const sp::MisArgs* me, const sp::SpecArgs* spc,
               const sp::GlassArgs* gls, const sp::EnvArgs* env, const sp::GlossArgs* glo, const sp::TexArgs* tex, const sp::NmapArgs* nmp, const sp::NormArgs* nrm, const sp::CamArgs* cam, F&& f) {
	with_accum(prog, ad, [&](const auto&... acc) {
		auto est = [&](const auto&... e) {
			constexpr bool tables = sizeof...(e) == 0 || sp::IsMis<std::decay_t<decltype(e)>...>::value;
			auto tail = [&](const auto&... t) {
				auto last = [&](const auto&... u) {
					if (cam) f(acc..., e..., t..., u..., *cam);
					else f(acc..., e..., t..., u...);
				};
				// a normal-mapped pack always carries vertex normals (the scene's or zeros): its packs without NormArgs are not built
				if constexpr (sp::IsNmap<std::decay_t<decltype(t)>...>::value) last(*nrm);
				else {
					if constexpr (tables) { if (nrm) { last(*nrm); return; } }
					last();
				}
			};
			if constexpr (tables) { if (nmp) { tail(*nmp); return; } }      // the normal map carries the UV table, the atlas and all they carry
			if constexpr (tables) { if (tex) { tail(*tex); return; } }      // the UV table and the atlas carry the roughness table and all it carries
			if constexpr (tables) { if (glo) { tail(*glo); return; } }      // the roughness table carries the map and both tables
			if constexpr (tables) { if (env) { tail(*env); return; } }      // the environment map carries the dielectric and the specular table
			if constexpr (tables) { if (gls) { tail(*gls); return; } }      // the dielectric table carries the specular one
			if constexpr (tables) { if (spc) { tail(*spc); return; } }
			tail();
		};
		if (me) est(*me);
		else if (ne) est(*ne);
		else est();
	});
}

// f(Shape<R, SPLIT, SCAN>{}) for a two-stage variant's scan shape (scan 4: the 512-thread shape of scan 3, set by launch_render).
// The one-scan kernels (k_hit_filter, k_flat_filter) take <R, SCAN> of the same shape.
template <int R_, bool SPLIT_, int SCAN_> struct Shape {
	static constexpr int R = R_, SCAN = SCAN_;
	static constexpr bool SPLIT = SPLIT_;
};
template <typename F>
void with_scan_shape(const TwoStage& ts, F&& f) {
	if (ts.scan == 3) f(Shape<1, false, 3>{});
	else if (ts.scan == 4) f(Shape<1, false, 4>{});
	else f(Shape<4, true, 2>{});
}

// ---- the flag rules that launch_render and accum_begin share (a begin checks as a path-tracing render would: the step would
// refuse as well, so it says so at once)
// per-sample camera rays: path tracing behind a camera, with the carried variants, without primary-hit reuse (the
// primary ray is no longer shared by the samples); flat and hit queries ignore the flag
int check_camera_rule(sphip_ctx* c, int flags, int variant, int mode, bool have_cam) {
	if (mode != SPHIP_MODE_PT || !(flags & SPHIP_FLAG_CAMERA_SAMPLES)) return SPHIP_OK;
	if (!have_cam)
		return fail(c, SPHIP_E_INVALID, "SPHIP_FLAG_CAMERA_SAMPLES needs a camera (sphip_render_camera, sphip_accum_begin[_adaptive] with cam), not rays");
	if (flags & SPHIP_FLAG_PRIMARY_REUSE)
		return fail(c, SPHIP_E_INVALID, "SPHIP_FLAG_CAMERA_SAMPLES and SPHIP_FLAG_PRIMARY_REUSE exclude each other (every sample has its own primary ray)");
	if (!variant_carried(variant))
		return fail(c, SPHIP_E_INVALID, "SPHIP_FLAG_CAMERA_SAMPLES is not available with kernel variant %d (%s)", variant, kVariants[variant].name);
	return SPHIP_OK;
}

// the per-triangle tables: specular reflection and smooth shading (5.8; variants 1, 8 and 16 only: 2 and 15 are
// A/B scans).  Path tracing with the plain estimator or with NEE|MIS, with the feature's variants, once its table is set; the flat pass
// has no use for them and says so; hit queries ignore the flags
struct TableRule { int bit; const char* flag; bool (*variant_ok)(int); bool sphip_ctx::*have; const char* needs; int with = 0; const char* with_flag = nullptr; };
const TableRule kTableRules[] = {
	{ SPHIP_FLAG_SPECULAR, "SPHIP_FLAG_SPECULAR", variant_carried, &sphip_ctx::have_spec, "a specular table (sphip_set_specular)" },
	{ SPHIP_FLAG_SMOOTH, "SPHIP_FLAG_SMOOTH", variant_smooth, &sphip_ctx::have_vnorm, "vertex normals (sphip_set_vertex_normals)" },
	{ SPHIP_FLAG_DIELECTRIC, "SPHIP_FLAG_DIELECTRIC", variant_smooth, &sphip_ctx::have_glass, "a dielectric table (sphip_set_dielectric)" },
	// environment lighting follows the same rules with the context's map for a table
	{ SPHIP_FLAG_ENVIRONMENT, "SPHIP_FLAG_ENVIRONMENT", variant_smooth, &sphip_ctx::have_env, "an environment map (sphip_set_environment)" },
	// glossy reflection roughens the mirror lobe: valid only together with SPHIP_FLAG_SPECULAR, as MIS is with NEE
	{ SPHIP_FLAG_GLOSSY, "SPHIP_FLAG_GLOSSY", variant_smooth, &sphip_ctx::have_rough, "a roughness table (sphip_set_roughness)", SPHIP_FLAG_SPECULAR, "SPHIP_FLAG_SPECULAR" },
	// textures need two things, asked for in this order: the scene's UV table and the context's atlas
	{ SPHIP_FLAG_TEXTURE, "SPHIP_FLAG_TEXTURE", variant_smooth, &sphip_ctx::have_uv, "a UV table (sphip_set_uv)" },
	{ SPHIP_FLAG_TEXTURE, "SPHIP_FLAG_TEXTURE", variant_smooth, &sphip_ctx::have_tex, "an atlas (sphip_set_texture)" },
	// normal mapping likewise: the scene's UV table, then the context's normal map
	{ SPHIP_FLAG_NORMAL_MAP, "SPHIP_FLAG_NORMAL_MAP", variant_smooth, &sphip_ctx::have_uv, "a UV table (sphip_set_uv)" },
	{ SPHIP_FLAG_NORMAL_MAP, "SPHIP_FLAG_NORMAL_MAP", variant_smooth, &sphip_ctx::have_nmap, "a normal map (sphip_set_normal_map)" },
};
int check_table_rule(sphip_ctx* c, const TableRule& r, int flags, int variant, int mode) {
	if (mode == kModeHits || !(flags & r.bit)) return SPHIP_OK;
	if (mode == SPHIP_MODE_FLAT) return fail(c, SPHIP_E_INVALID, "%s is valid for SPHIP_MODE_PT only", r.flag);
	if ((flags & SPHIP_FLAG_NEE) && !(flags & SPHIP_FLAG_MIS))
		return fail(c, SPHIP_E_INVALID, "%s works with the plain estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS, not with SPHIP_FLAG_NEE alone", r.flag);
	if (!r.variant_ok(variant)) return fail(c, SPHIP_E_INVALID, "%s is not available with kernel variant %d (%s)", r.flag, variant, kVariants[variant].name);
	if (r.with && !(flags & r.with)) return fail(c, SPHIP_E_INVALID, "%s needs %s", r.flag, r.with_flag);
	if (!(c->*r.have)) return fail(c, SPHIP_E_STATE, "%s needs %s", r.flag, r.needs);
	return SPHIP_OK;
}
// the whole chain, in the order in which a call that breaks several rules hears of them: the camera, then the tables as listed
int check_feature_rules(sphip_ctx* c, int flags, int variant, int mode, bool have_cam) {
	int rc = check_camera_rule(c, flags, variant, mode, have_cam);
	for (const TableRule& r : kTableRules) if (!rc) rc = check_table_rule(c, r, flags, variant, mode);
	return rc;
}

// what sphip_get_stats reports of the last launch on c
void note_render(sphip_ctx* c, hipStream_t st, size_t n_pixels, int variant) {
	c->have_render = true;
	c->last_stream = st;
	c->stats.n_pixels = n_pixels;
	c->stats.n_tris = c->n_tris;
	c->stats.kernel_variant = (uint32_t)variant;
}

// ---- One render launch.  RenderCall is what the entry points hand launch_render: the rays, the outputs and the stream, then what only
// some of them set.  prog: progressive accumulation (path tracing only): the launch renders global samples [prog->sample_base,
// prog->sample_base + n_samples) into the running sum prog->sum, and accum receives the mean of all of them; adapt: the same over the
// active list of adaptive sampling; cam: the camera of SPHIP_FLAG_CAMERA_SAMPLES; src: the source triangles of a hit query
struct RenderCall {
	const void* rays; size_t n_rays, n_samples; uint64_t seed; int mode, flags; void* rgba; void* accum; hipStream_t st;
	const sphip_shard* shard = nullptr; const int* src = nullptr;
	const sp::AccumArgs* prog = nullptr; const sp::AdaptArgs* adapt = nullptr; const sp::CamArgs* cam = nullptr;
};
// what the steps hand on: check_render's verdict (the variant, its shape, the feature bits), plan_render's plan, bind_render's arguments
struct Launch {
	int variant = 0; TwoStage ts{}; Features f{};
	uint32_t bthreads = 256;                 // threads per workgroup of the variant's kernels
	LaunchPlan p;
	sp::KArgs a{}; sp::ScanSrc src{}; sp::BvhArgs B{}; sp::AdaptArgs ad{}; sp::NormArgs nra{};
	int2* hist = nullptr; float* acc = nullptr;   // the work buffer's path history and accumulator
	sp::MisArgs est{};                       // the light table; handed on as NeeArgs or as MisArgs
	sp::NmapArgs tab{};                      // the per-triangle tables, the map, the atlas and the normal map; handed on as SpecArgs, GlassArgs, EnvArgs, GlossArgs, TexArgs or NmapArgs
};

// ---- step 1, check: refuse what cannot be rendered and name what will be.  The order is behaviour (a call that is wrong twice hears of
// the first): no scene; null rays or output; n_rays; mode; a hit query's distance output; n_samples; progressive accumulation's mode and
// sum, then its sample total; shard.tile_px; the default scan's 2^26 triangles; a retired variant; MIS without NEE; under NEE the scene's
// emittances (ensure_lights builds the light table here to keep that place: before the feature rules); the camera rule and the table rules
// (check_feature_rules); and only then anything on the stream: an environment render's zero rows and flagged light table
int check_render(sphip_ctx* c, const RenderCall& r, Launch& L) {
	const int mode = r.mode, flags = r.flags;
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "render called before a scene was set");
	if (!r.rays || !r.rgba) return fail(c, SPHIP_E_INVALID, "null ray or output pointer");
	if (r.n_rays == 0 || r.n_rays > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "n_rays %zu out of range", r.n_rays);
	if (mode != SPHIP_MODE_FLAT && mode != SPHIP_MODE_PT && mode != kModeHits) return fail(c, SPHIP_E_INVALID, "unknown mode %d", mode);
	if (mode == kModeHits && !r.accum) return fail(c, SPHIP_E_INVALID, "null distance output");
	const bool pt = mode == SPHIP_MODE_PT;
	if (pt && (r.n_samples == 0 || r.n_samples > 0x7fffffffull))
		return fail(c, SPHIP_E_INVALID, "n_samples must be in [1, 2^31) (the reference divides by it, cpu_renderer.cpp:77)");
	if (r.prog && (!pt || !r.prog->sum)) return fail(c, SPHIP_E_INVALID, "progressive accumulation needs path tracing and a sum buffer");
	if (r.prog && (uint64_t)r.prog->sample_base + r.n_samples > 0x7fffffffull)
		return fail(c, SPHIP_E_INVALID, "sample_base + n_samples = %llu: the total must stay below 2^31", (unsigned long long)r.prog->sample_base + r.n_samples);
	int rc;
	if ((rc = ensure(c, c->counter, 16 * sizeof(unsigned long long)))) return rc;
	if (r.shard && r.shard->tile_px == 0) return fail(c, SPHIP_E_INVALID, "shard.tile_px must be > 0");
	const int variant = L.variant = pick_variant(flags, c->n_tris);
	if (variant == 16 && c->n_tris >= (1ull << sp::kMIdxBits))
		return fail(c, SPHIP_E_INVALID, "rpl_cylm handles scenes of fewer than 2^%u triangles (this one has %zu); use rpl_cylw4s", sp::kMIdxBits, c->n_tris);
	if (!variant_carried(variant))
		return fail(c, SPHIP_E_INVALID, "kernel variant %d (%s) is retired: libspath_hip no longer carries it", variant, kVariants[variant].name);
	L.ts = kVariants[variant].ts;
	// the features are those of path tracing: flat and hit queries ignore the flags.  MIS is a form of NEE
	auto on = [&](int bit) { return pt && (flags & bit); };
	const Features f = L.f = { on(SPHIP_FLAG_NEE), on(SPHIP_FLAG_MIS), on(SPHIP_FLAG_SPECULAR), on(SPHIP_FLAG_DIELECTRIC), on(SPHIP_FLAG_ENVIRONMENT),
	                           on(SPHIP_FLAG_SMOOTH), on(SPHIP_FLAG_CAMERA_SAMPLES), r.adapt != nullptr, r.prog != nullptr, on(SPHIP_FLAG_GLOSSY),
	                           on(SPHIP_FLAG_TEXTURE), on(SPHIP_FLAG_NORMAL_MAP) };
	if (f.mis && !f.nee) return fail(c, SPHIP_E_INVALID, "SPHIP_FLAG_MIS needs SPHIP_FLAG_NEE");
	if (f.nee && (rc = ensure_lights(c, r.st))) return rc;
	if ((rc = check_feature_rules(c, flags, variant, mode, r.cam != nullptr))) return rc;
	// environment lighting stands zeros in for either table whose flag is off; under NEE|MIS the estimator reads the flagged light table
	// and so does glossy reflection for the dielectric table, and its black map for the environment; a textured render does both, and
	// the zeros are its roughness table too when SPHIP_FLAG_GLOSSY is not set
	// a normal-mapped render is a textured one with these stand-ins, and its own: zero vertex normals and the white texel
	const bool tx = f.tex || f.nmap;
	if ((f.env || f.gloss || tx) && (!f.spec || !f.glass || (tx && !f.gloss)) && (rc = ensure_zero_rows(c, r.st))) return rc;
	if (f.env && f.nee && (rc = ensure_env_lights(c, r.st))) return rc;
	if ((f.gloss || tx) && !f.env && (rc = ensure_black_map(c, r.st))) return rc;
	if (f.nmap && !f.smooth && (rc = ensure_zero_vnorm(c, r.st))) return rc;
	if (f.nmap && !f.tex && (rc = ensure_white_texel(c, r.st))) return rc;
	return SPHIP_OK;
}

// ---- step 2, plan: zero the scan counter, derive the default scan's record stream on first use (it decides between the scan's two
// shapes, and so the threads per workgroup), then plan_launch (sp_host_plan.h): sample chunks, grids, work slots
int plan_render(sphip_ctx* c, const RenderCall& r, Launch& L) {
	HIP_TRY(c, hipMemsetAsync(c->counter.p, 0, 16 * sizeof(unsigned long long), r.st));
	if (L.ts.scan == 3) {
		if (const int rc = ensure_cylm(c, r.st)) return rc;
		if (c->cylm_wide) { L.ts.scan = 4; L.bthreads = sp::cylm512::kMThreads; }      // the 512-thread shape of the same scan (sp_cylm_both.h)
	}
	const uint32_t forced = ((uint32_t)r.flags & SPHIP_FLAG_CHUNKS_MASK) >> SPHIP_FLAG_CHUNKS_SHIFT;
	L.p = plan_launch(r.n_rays, r.n_samples, forced, r.mode == SPHIP_MODE_PT, L.ts, L.bthreads, L.f, c->samp.cap, c->work.cap, []() -> int64_t {
		size_t free_b = 0, total_b = 0;
		return hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (int64_t)free_b : -1;
	});
	if (L.p.too_large) return fail(c, SPHIP_E_INVALID, "n_rays %zu too large for one launch of this kernel variant; shard the frame", r.n_rays);
	return SPHIP_OK;
}

// ---- step 3, bind: the buffers the plan asks for and the kernels' argument structs
int bind_render(sphip_ctx* c, const RenderCall& r, Launch& L) {
	const Features& f = L.f;
	const LaunchPlan& p = L.p;
	int rc;
	sp::KArgs& a = L.a;
	a.rays = (const float*)r.rays; a.out_rgba = (uint32_t*)r.rgba; a.out_accum = (float*)r.accum;
	a.scan = (const float4*)c->scan.p; a.tris = (const float*)c->tris.p; a.mats = (const float*)c->mats.p;
	a.scans = (unsigned long long*)c->counter.p;
	a.n_rays = (uint32_t)r.n_rays; a.n_tris = (uint32_t)c->n_tris; a.n_samples = (uint32_t)r.n_samples;
	a.flags = (uint32_t)r.flags; a.seed = r.seed;
	a.pixel_base = 0; a.tile_px = r.n_rays; a.tile_stride_px = 0;
	if (r.shard) { a.pixel_base = r.shard->pixel_base; a.tile_px = r.shard->tile_px; a.tile_stride_px = r.shard->tile_stride_px; }
	const uint64_t n_total = (r.prog ? (uint64_t)r.prog->sample_base : 0) + r.n_samples;
	a.inv_n = (float)(1.0 / (double)(n_total ? n_total : 1));          // cpu_renderer.cpp:77 (all samples so far when accumulating)
	if (p.chunks > 1) {
		a.n_chunks = p.chunks; a.px_blocks = p.px_blocks; a.samp_stride = p.samp_stride;
		if ((rc = ensure(c, c->samp, (size_t)p.samp_bytes))) return rc;
		a.samp = (float*)c->samp.p;
	}
	if (r.adapt) L.ad = *r.adapt;
	if (r.mode == SPHIP_MODE_PT && L.ts.R != 0) {              // the two-stage kernels' work-side buffers: n_work slots of p.slot bytes each
		if ((rc = ensure(c, c->work, (size_t)p.n_work * p.slot.work))) return rc;
		if (p.slot.adp_wst && (rc = ensure(c, c->adp_wst, (size_t)p.n_work * p.slot.adp_wst))) return rc;
		if (p.slot.env_M && (rc = ensure(c, c->env_M, (size_t)p.n_work * p.slot.env_M))) return rc;
		if (p.slot.tex_A && (rc = ensure(c, c->tex_A, (size_t)p.n_work * p.slot.tex_A))) return rc;
		L.hist = (int2*)c->work.p;
		L.acc = (float*)((char*)c->work.p + (size_t)p.n_work * kSlotHist);
		L.est.L = (float*)((char*)c->work.p + (size_t)p.n_work * (kSlotHist + kSlotAcc));     // NEE: L[4][3][n_work]; MIS: D[5][3][n_work]
		L.ad.wst = (double*)c->adp_wst.p;
		L.tab.M = (float*)c->env_M.p;
		L.tab.A = (float*)c->tex_A.p;
	}
	if (L.ts.scan == 2 && (rc = ensure_cyl(c, r.st))) return rc;
	L.src.cyl.rec = (const float4*)c->cyl_rec.p; L.src.cyl.hdr = (const uint32_t*)c->cyl_hdr.p;
	L.src.cylm.rec = (const float4*)c->cylm_rec.p; L.src.cylm.hdr = (const uint32_t*)c->cylm_hdr.p; L.src.cylm.big = (const float4*)c->cylm_big.p;
	if (L.variant == kVariantAccel) {
		if ((rc = ensure_bvh(c, r.st))) return rc;
		L.B.nodes = (const float4*)c->bvh_nodes.p; L.B.leaf_rec = (const float4*)c->bvh_rec.p; L.B.leaf_idx = (const int*)c->bvh_idx.p;
		L.B.n_leaves = c->bvh_leaves; L.B.first_leaf = c->bvh_leaves; L.B.meta = (const uint32_t*)c->bvh_meta.p;
	}
	if (f.nee) {
		// an environment map with an entry in the light table: the estimator reads the flagged table (a black map adds none)
		const bool flagged = f.env && c->env_nee_n != c->nee_n;
		const uint32_t n = flagged ? c->env_nee_n : c->nee_n;
		const LightView v = light_view(flagged ? c->env_tab.p : c->nee_tab.p, n);
		L.est.cdf = v.cdf; L.est.tri = v.tri; L.est.ipdf = v.ipdf; L.est.tipdf = v.tipdf; L.est.n = n; L.est.W = flagged ? c->env_W : c->nee_W;
	}
	// the tables whose flags are set, the zeros for the others (read after ensure_zero_rows: it may have allocated them)
	L.tab.spec = (const float4*)(f.spec ? c->spec.p : c->spec_zero.p);
	L.tab.glass = (const float4*)(f.glass ? c->glass.p : c->spec_zero.p);
	if (f.env) L.tab.env = sp::EnvMap{ (const float*)c->env_tex.p, (const double*)c->env_rc.p, (const double*)c->env_marg.p, (const float*)c->env_tpdf.p, c->env_T, c->env_n };
	else if (f.gloss || f.tex || f.nmap) L.tab.env = sp::EnvMap{ (const float*)c->env_black.p, (const double*)c->env_black.p, (const double*)c->env_black.p, (const float*)c->env_black.p, 0.0, 1u };
	L.tab.rough = (const float*)(f.gloss ? c->rough.p : c->spec_zero.p);
	L.tab.uv = (const float*)c->uv.p; L.tab.atlas = (const float*)c->atlas.p; L.tab.tw = c->tex_w; L.tab.th = c->tex_h;
	if (f.nmap && !f.tex) { L.tab.atlas = (const float*)c->tex_white.p; L.tab.tw = L.tab.th = 1u; }
	L.tab.nmap = (const float*)c->nmap.p; L.tab.nw = c->nmap_w; L.tab.nh = c->nmap_h;
	L.nra.vnorm = (const float*)(f.nmap && !f.smooth ? c->vnorm_zero.p : c->vnorm.p);
	return SPHIP_OK;
}

// ---- step 4, dispatch: ev_k0, the primary-hit pre-pass, the kernel the variant, the mode and the feature bits select, the resolve, ev_k1
int dispatch_render(sphip_ctx* c, const RenderCall& r, Launch& L) {
	const Features& f = L.f;
	const TwoStage& ts = L.ts;
	const bool is_ts = ts.R != 0;
	const int variant = L.variant, mode = r.mode;
	hipStream_t st = r.st;
	sp::KArgs& a = L.a;
	const dim3 block(256), block_ts(L.bthreads), grid(L.p.grid), grid_px(L.p.grid_px), grid_pt(L.p.grid_pt);
	const unsigned int* bnd = (const unsigned int*)c->bounds.p;
	HIP_TRY(c, hipEventRecord(c->ev_k0, st));
	// the closest-hit scan alone with a two-stage variant, R pixels per lane: hit queries and the primary-hit pre-pass
	auto hit_filter = [&](const sp::KArgs& ka, const int* src_idx, int* oi, float* od) {
		with_scan_shape(ts, [&](auto shape) {
			using S = decltype(shape);
			hipLaunchKernelGGL((sp::k_hit_filter<S::R, S::SCAN>), grid_px, block_ts, 0, st, ka, L.src, bnd, src_idx, oi, od);
		});
	};
	// primary-hit reuse with a two-stage kernel: one closest-hit scan per PIXEL first (R pixels per lane, the same scan family),
	// whatever the number of samples and sample chunks; the path-tracing launch then starts every sample from that hit
	bool prim_pass = false;
	if (mode == SPHIP_MODE_PT && is_ts && (r.flags & SPHIP_FLAG_PRIMARY_REUSE)) {
		if (const int rc = ensure(c, c->prim, r.n_rays * 8)) return rc;
		int* oi = (int*)c->prim.p; float* od = (float*)((char*)c->prim.p + r.n_rays * 4);
		sp::KArgs h = a;
		h.n_chunks = 0; h.samp = nullptr;
		hit_filter(h, nullptr, oi, od);
		a.prim_idx = oi; a.prim_d = od;
		prim_pass = true;
	}
	// the pack's carriers: the estimator rides as NeeArgs or MisArgs, the tables as the base of EnvArgs that the flags reach
	const sp::NeeArgs* ne = f.nee ? &L.est : nullptr;
	const bool tx = f.tex || f.nmap;
	const sp::SpecArgs* spc = f.spec && !f.glass && !f.env && !f.gloss && !tx ? &L.tab : nullptr;
	const sp::GlassArgs* gls = f.glass && !f.env && !f.gloss && !tx ? &L.tab : nullptr;
	const sp::EnvArgs* env = f.env && !f.gloss && !tx ? &L.tab : nullptr;
	const sp::GlossArgs* glo = f.gloss && !tx ? &L.tab : nullptr;
	const sp::AdaptArgs* adp = f.adapt ? &L.ad : nullptr;
	auto pt_pack = [&](auto&& fn) { with_pack(r.prog, adp, ne, f.mis ? &L.est : nullptr, spc, gls, env, glo, f.tex && !f.nmap ? &L.tab : nullptr, f.nmap ? &L.tab : nullptr, f.smooth || f.nmap ? &L.nra : nullptr, f.cam ? r.cam : nullptr, fn); };
	// k_accel in mode M (0 flat, 1 path tracing, 2 hits); the exact-only kernels of variant 1 (rpl_sload) or 2 (rpl_lds)
	auto accel = [&](auto mode_c, const int* src_idx, int* oi, float* od, const auto&... p) {
		hipLaunchKernelGGL((sp::k_accel<decltype(mode_c)::value, std::decay_t<decltype(p)>...>), grid, block, 0, st, a, L.B, src_idx, oi, od, p...);
	};
	auto with_exact = [&](auto&& fn) {
		if (variant == 2) fn(std::integral_constant<int, 2>{});
		else fn(std::integral_constant<int, 1>{});
	};
	if (mode == kModeHits) {
		int* oi = (int*)r.rgba; float* od = (float*)r.accum;
		if (variant == kVariantAccel) accel(std::integral_constant<int, 2>{}, r.src, oi, od);
		else if (is_ts) hit_filter(a, r.src, oi, od);
		else with_exact([&](auto v) { hipLaunchKernelGGL((sp::k_hit<decltype(v)::value>), grid, block, 0, st, a, r.src, oi, od); });
	} else if (mode == SPHIP_MODE_FLAT) {
		if (variant == kVariantAccel) accel(std::integral_constant<int, 0>{}, nullptr, nullptr, nullptr);
		else if (is_ts) with_scan_shape(ts, [&](auto shape) {
			using S = decltype(shape);
			hipLaunchKernelGGL((sp::k_flat_filter<S::R, S::SCAN>), grid_px, block_ts, 0, st, a, L.src, bnd);
		});
		else with_exact([&](auto v) { hipLaunchKernelGGL((sp::k_flat<decltype(v)::value>), grid, block, 0, st, a); });
	} else if (variant == kVariantAccel) {
		pt_pack([&](const auto&... p) { accel(std::integral_constant<int, 1>{}, nullptr, nullptr, nullptr, p...); });
	} else if (is_ts) {
		with_scan_shape(ts, [&](auto shape) {
			using S = decltype(shape);
			pt_pack([&](const auto&... p) {
				// smooth shading and transparency are built for the default scan's two shapes only (checked above)
				if constexpr (S::SCAN >= 3 || !(sp::IsNorm<std::decay_t<decltype(p)>...>::value || sp::IsGlass<std::decay_t<decltype(p)>...>::value))
					hipLaunchKernelGGL((sp::k_pt_filter<S::R, S::SPLIT, S::SCAN, std::decay_t<decltype(p)>...>), grid_pt, block_ts, 0, st,
					                   a, L.src, bnd, L.hist, L.acc, L.p.n_work, p...);
			});
		});
	} else {
		with_exact([&](auto v) {
			pt_pack([&](const auto&... p) {
				if constexpr (decltype(v)::value == 1 || !(sp::IsNorm<std::decay_t<decltype(p)>...>::value || sp::IsGlass<std::decay_t<decltype(p)>...>::value))   // smooth shading, transparency: variant 1 only (checked above)
					hipLaunchKernelGGL((sp::k_pt<decltype(v)::value, std::decay_t<decltype(p)>...>), grid, block, 0, st, a, p...);
			});
		});
	}
	if (L.p.chunks > 1)
		with_accum(r.prog, adp, [&](const auto&... q) {
			hipLaunchKernelGGL((sp::k_resolve<std::decay_t<decltype(q)>...>), dim3((unsigned)((r.n_rays + 255) / 256)), block, 0, st, a, q...);
		});
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(c->ev_k1, st));
	note_render(c, st, r.n_rays, variant);
	c->stats.n_launches = L.p.n_launches + (prim_pass ? 1u : 0u);
	return SPHIP_OK;
}

int launch_render(sphip_ctx* c, RenderCall r) {
	if (r.adapt) r.prog = r.adapt;                  // an adaptive launch is a progressive one over the active list (sp_kernels.h)
	Launch L;
	int rc;
	if ((rc = check_render(c, r, L)) || (rc = plan_render(c, r, L)) || (rc = bind_render(c, r, L))) return rc;
	return dispatch_render(c, r, L);
}

// the viewport constants of view::camera::get_viewport (view.h:101-108: `real` (float) variables initialised from double expressions);
// the shard fields are the whole image
sp::ViewArgs view_args(const sphip_camera* cam) {
	sp::ViewArgs v{};
	const float x_size = (float)(1.0 * (double)cam->res_x / (double)cam->res_y), y_size = 1.0f;
	v.x_max = (float)((double)x_size / 2.0);
	v.x_step = x_size / (float)cam->res_x;
	v.h_x_step = (float)((double)v.x_step / 2.0);
	v.y_max = (float)((double)y_size / 2.0);
	v.y_step = y_size / (float)cam->res_y;
	v.h_y_step = (float)((double)v.y_step / 2.0);
	v.focal = cam->focal; v.cos_y = cam->cos_y; v.sin_y = cam->sin_y; v.cos_x = cam->cos_x; v.sin_x = cam->sin_x;
	v.px = cam->pos[0]; v.py = cam->pos[1]; v.pz = cam->pos[2];
	v.res_x = cam->res_x; v.res_y = cam->res_y;
	v.n_local = cam->res_x * cam->res_y;
	v.pixel_base = 0; v.tile_px = v.n_local; v.tile_stride_px = 0;
	return v;
}

// the trailing kernel argument of per-sample camera rays (sp_kernels.h CamArgs): the camera's viewport constants and a lens
sp::CamArgs cam_args_of(const sphip_camera* cam, const sphip_lens& lens) {
	sp::CamArgs ca{};
	ca.v = view_args(cam);
	ca.aperture = lens.aperture;
	ca.focus_dist = lens.focus_dist;
	return ca;
}

// ---- view::camera::get_viewport on the device for the pixels of a shard (sp_kernels.h: k_viewport)
int launch_viewport(sphip_ctx* c, const sphip_camera* cam, void* d_rays, hipStream_t st, const sphip_shard* shard = nullptr, size_t n_local = 0) {
	if (!cam || !d_rays) return fail(c, SPHIP_E_INVALID, "null camera or ray pointer");
	if (cam->res_x == 0 || cam->res_y == 0 || (uint64_t)cam->res_x * cam->res_y > 0xffffffffull)
		return fail(c, SPHIP_E_INVALID, "bad viewport size %ux%u", cam->res_x, cam->res_y);
	sp::ViewArgs v = view_args(cam);
	const uint32_t n = shard ? (uint32_t)n_local : cam->res_x * cam->res_y;
	v.n_local = n;
	if (shard) { v.pixel_base = shard->pixel_base; v.tile_px = shard->tile_px; v.tile_stride_px = shard->tile_stride_px; }
	else { v.pixel_base = 0; v.tile_px = n; v.tile_stride_px = 0; }
	if (n == 0) return SPHIP_OK;
	hipLaunchKernelGGL(sp::k_viewport, dim3((n + 255) / 256), dim3(256), 0, st, v, (float*)d_rays);
	HIP_TRY(c, hipGetLastError());
	return SPHIP_OK;
}


// =====================================================================================================================
// All GPUs of a node behind one context (include/spath_hip.h: sphip_create_multi).  The reference has no multi-device
// code; what is sharded is the pixel loop of cpu_renderer.cpp:70-79,118-184 (pixels are independent), behind the same
// renderer::render / render_flat calls (src/renderer.h:31-32).
// =====================================================================================================================

// ---- the row-tile plan
int plan_tile_rows(size_t height, int n_dev) {
	for (int tr = 8; tr >= 1; --tr)
		if (height % (size_t)tr == 0 && (height / (size_t)tr) % (size_t)n_dev == 0) return tr;
	return 8;
}

struct RowPlan {
	size_t w, h, tile_rows, tile_px, n_tiles, npix;
	int g;
	RowPlan(size_t w_, size_t h_, int g_, size_t tr) : w(w_), h(h_), tile_rows(tr), tile_px(tr * w_), n_tiles((h_ + tr - 1) / tr), npix(w_ * h_), g(g_) {}
	size_t n_rays(int rank) const {
		size_t n = 0;
		for (size_t t = (size_t)rank; t < n_tiles; t += (size_t)g) n += std::min(tile_px, npix - t * tile_px);
		return n;
	}
	size_t max_rays() const { size_t m = 0; for (int r = 0; r < g; ++r) m = std::max(m, n_rays(r)); return m; }
	sphip_shard shard(int rank) const { return sphip_shard{ (uint64_t)rank * tile_px, (uint64_t)tile_px, (uint64_t)g * tile_px }; }
	// the image-order pixel of local index i of that shard
	size_t pixel(int rank, size_t i) const { const sphip_shard sh = shard(rank); return sh.pixel_base + (i / sh.tile_px) * sh.tile_stride_px + i % sh.tile_px; }
};

// ---- RCCL, loaded on first use: the single-GPU path (and every process that never creates a multi-device context) does not
// depend on librccl being present
typedef int (*nccl_init_all_t)(void**, int, const int*);
typedef int (*nccl_comm_destroy_t)(void*);
typedef int (*nccl_group_t)(void);
typedef int (*nccl_send_t)(const void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_recv_t)(void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*nccl_errstr_t)(int);
struct Rccl {
	nccl_init_all_t init_all = nullptr; nccl_comm_destroy_t destroy = nullptr; nccl_group_t group_start = nullptr, group_end = nullptr;
	nccl_send_t send = nullptr; nccl_recv_t recv = nullptr; nccl_errstr_t errstr = nullptr;
} g_rccl;
constexpr int kNcclUint8 = 1;      // ncclDataType_t::ncclUint8 (rccl.h)

// (once per process, under a lock: contexts may be created from several threads; the table is never changed afterwards and the
// library stays loaded)
void* load_rccl() {
	static std::mutex mu;
	static void* loaded = nullptr;
	std::lock_guard<std::mutex> lock(mu);
	if (loaded) return loaded;
	const char* names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
	for (const char* n : names) {
		void* h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
		if (!h) continue;
		g_rccl.init_all = (nccl_init_all_t)dlsym(h, "ncclCommInitAll");
		g_rccl.destroy = (nccl_comm_destroy_t)dlsym(h, "ncclCommDestroy");
		g_rccl.group_start = (nccl_group_t)dlsym(h, "ncclGroupStart");
		g_rccl.group_end = (nccl_group_t)dlsym(h, "ncclGroupEnd");
		g_rccl.send = (nccl_send_t)dlsym(h, "ncclSend");
		g_rccl.recv = (nccl_recv_t)dlsym(h, "ncclRecv");
		g_rccl.errstr = (nccl_errstr_t)dlsym(h, "ncclGetErrorString");
		if (g_rccl.init_all && g_rccl.destroy && g_rccl.group_start && g_rccl.group_end && g_rccl.send && g_rccl.recv) { loaded = h; return h; }
		g_rccl = Rccl{};
		dlclose(h);
	}
	return nullptr;
}

// Whatever goes wrong on one device, no device is left with work in flight when the call returns: the next call may free or
// regrow the buffers that work reads and writes.
void drain_all(sphip_ctx* c) {
	for (sphip_ctx* k : c->kids)
		if (hipSetDevice(k->device) == hipSuccess && k->own_stream) (void)hipStreamSynchronize(k->own_stream);
	(void)hipGetLastError();
}

// Per-device arrays (a buffer of every child, elem_bytes per pixel in its shard's order) read back and put in image order in the
// host arrays `out`.  A query, not the hot path: one wait per device for all the arrays.
struct ShardArray { DevBuf sphip_ctx::*buf; size_t elem_bytes; void* out; };
int read_shards(sphip_ctx* c, const RowPlan& plan, const std::vector<ShardArray>& arrays) {
	std::vector<std::vector<char>> loc(arrays.size());
	for (int r = 0; r < plan.g; ++r) {
		sphip_ctx* k = c->kids[(size_t)r];
		const size_t n = plan.n_rays(r);
		if (n == 0) continue;
		HIP_TRY(c, hipSetDevice(k->device));
		for (size_t a = 0; a < arrays.size(); ++a) {
			loc[a].resize(n * arrays[a].elem_bytes);
			HIP_TRY(c, hipMemcpyAsync(loc[a].data(), (k->*arrays[a].buf).p, loc[a].size(), hipMemcpyDeviceToHost, k->own_stream));
		}
		HIP_TRY(c, hipStreamSynchronize(k->own_stream));
		for (size_t i = 0; i < n; ++i)
			for (size_t a = 0, p = plan.pixel(r, i); a < arrays.size(); ++a)
				std::memcpy((char*)arrays[a].out + p * arrays[a].elem_bytes, &loc[a][i * arrays[a].elem_bytes], arrays[a].elem_bytes);
	}
	return SPHIP_OK;
}

// Device r's n pixels (and float triples) -> slot r of the first device's gather buffers, in stream order behind its kernels;
// ev_tile[r] marks their arrival.  A device listed twice, or the first device itself, makes it a local copy.  err receives an error.
int enqueue_peer_tile(sphip_ctx* c, sphip_ctx* err, int r, size_t n, size_t pad, bool with_accum) {
	sphip_ctx *k = c->kids[(size_t)r], *root = c->kids[0];
	auto copy = [&](const DevBuf& dst, const DevBuf& src, size_t elem) {
		char* d = (char*)dst.p + (size_t)r * pad * elem;
		if (k->device == root->device) return hipMemcpyAsync(d, src.p, n * elem, hipMemcpyDeviceToDevice, k->own_stream);
		return hipMemcpyPeerAsync(d, root->device, src.p, k->device, n * elem, k->own_stream);
	};
	HIP_TRY(err, copy(c->gath, k->rgba, 4));
	if (with_accum) HIP_TRY(err, copy(c->gath_acc, k->accum, 12));
	HIP_TRY(err, hipEventRecord(c->ev_tile[(size_t)r], k->own_stream));
	return SPHIP_OK;
}

int multi_set_scene(sphip_ctx* c, const float* tris, const float* mats, size_t n_tris) {
	const int g = (int)c->kids.size();
	std::vector<int> rcs((size_t)g, SPHIP_OK);
	std::vector<std::thread> th;
	for (int r = 0; r < g; ++r) th.emplace_back([&, r] { rcs[(size_t)r] = sphip_set_scene(c->kids[(size_t)r], tris, mats, n_tris); });   // every device holds the whole scene
	for (auto& t : th) t.join();
	for (int r = 0; r < g; ++r)
		if (rcs[(size_t)r]) return fail(c, rcs[(size_t)r], "device %d: %s", c->kids[(size_t)r]->device, c->kids[(size_t)r]->err.c_str());
	c->n_tris = n_tris;
	c->have_scene = true;
	drop_tables(c);
	return SPHIP_OK;
}

// What every device of a multi-device context keeps whole (a per-triangle table, the map, the atlas): set_child on each child, `have`
// being the context's flag for it and present whether the call sets one.  A device that refuses leaves no device with one: they must
// never differ.
template <typename SetChild>
int set_on_every_device(sphip_ctx* c, bool sphip_ctx::*have, bool present, SetChild&& set_child) {
	c->acc_stale = c->acc_on;
	c->*have = false;
	for (sphip_ctx* k : c->kids)
		if (const int rc = set_child(k)) {
			for (sphip_ctx* q : c->kids) q->*have = false;
			return fail(c, rc, "device %d: %s", k->device, k->err.c_str());
		}
	c->*have = present;
	return SPHIP_OK;
}

// Table `id` of kTriTables on one device (a single-device context, or a child): its floats per triangle from src, or no table with
// src == nullptr.  sync: src is borrowed host memory and must not outlive the call.
int put_table(sphip_ctx* c, int id, const void* src, hipMemcpyKind kind, hipStream_t st, bool sync) {
	DevBuf& buf = c->*kTableSlots[id].buf;
	bool& have = c->*kTableSlots[id].have;
	const size_t bytes = c->n_tris * (size_t)kTriTables[id].floats * 4;
	c->acc_stale = c->acc_on;                      // the running sum was rendered with the old table
	have = false;
	if (!src) return SPHIP_OK;
	int rc;
	if (kTriTables[id].zero_rows && (rc = ensure_zero_rows(c, st))) return rc;
	HIP_TRY(c, hipSetDevice(c->device));
	if ((rc = ensure(c, buf, bytes))) return rc;
	HIP_TRY(c, hipMemcpyAsync(buf.p, src, bytes, kind, st));
	if (sync) HIP_TRY(c, hipStreamSynchronize(st));
	have = true;
	return SPHIP_OK;
}

// sphip_set_X: in this order the context, the scene, the triangle limit, the rows (a refusal so far leaves the old table in place), then
// the table on the device or, validated once here, on every device
int set_table(sphip_ctx* c, int id, const float* src) {
	if (!c) return SPHIP_E_INVALID;
	const TriTable& t = kTriTables[id];
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "%s called before a scene was set", t.setter);
	if (src) {
		if (t.max_tris && c->n_tris >= t.max_tris) return fail(c, SPHIP_E_INVALID, t.too_large, c->n_tris);
		const size_t bad = first_bad_row(t, src, c->n_tris);
		if (bad < c->n_tris) return fail(c, SPHIP_E_INVALID, "%s", bad_row_message(t, src, bad).c_str());
	}
	if (c->kids.empty()) return put_table(c, id, src, hipMemcpyHostToDevice, c->own_stream, true);
	return set_on_every_device(c, kTableSlots[id].have, src != nullptr,
	                           [&](sphip_ctx* k) { return put_table(k, id, src, hipMemcpyHostToDevice, k->own_stream, true); });
}

// sphip_set_X_device: the rows are not validated; a scene beyond the triangle limit is refused, and like every call it leaves no table behind
int set_table_device(sphip_ctx* c, int id, const void* d_src, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	const TriTable& t = kTriTables[id];
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "%s_device called before a scene was set", t.setter);
	const bool big = d_src && t.max_tris && c->n_tris >= t.max_tris;
	const int rc = put_table(c, id, big ? nullptr : d_src, hipMemcpyDeviceToDevice, (hipStream_t)stream, false);
	return big ? fail(c, SPHIP_E_INVALID, t.too_large, c->n_tris) : rc;
}

// The tail of the host-pointer paths: n pixels of c->rgba (and, with out_f, the float triples of c->accum) to the caller, timed for
// sphip_get_stats; blocking, like every reference backend (main.cpp:70-83)
int download_frame(sphip_ctx* c, size_t n, uint8_t* out_rgba, float* out_f, hipStream_t st) {
	HIP_TRY(c, hipEventRecord(c->ev_d0, st));
	HIP_TRY(c, hipMemcpyAsync(out_rgba, c->rgba.p, n * 4, hipMemcpyDeviceToHost, st));
	if (out_f) HIP_TRY(c, hipMemcpyAsync(out_f, c->accum.p, n * 12, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipEventRecord(c->ev_d1, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	return SPHIP_OK;
}

// device r's rays of a frame, in its shard's order: its tiles of the caller's viewport (host array, one copy per tile), or,
// with rays == nullptr, generated on the device from cam
int deal_rays(sphip_ctx* k, const RowPlan& plan, int r, const float* rays, const sphip_camera* cam, void* d_rays, hipStream_t st) {
	if (rays) {
		size_t k0 = 0;
		for (size_t t = (size_t)r; t < plan.n_tiles; t += (size_t)plan.g) {
			const size_t cnt = std::min(plan.tile_px, plan.npix - t * plan.tile_px);
			HIP_TRY(k, hipMemcpyAsync((char*)d_rays + k0 * 24, rays + t * plan.tile_px * 6, cnt * 24, hipMemcpyHostToDevice, st));
			k0 += cnt;
		}
		return SPHIP_OK;
	}
	const sphip_shard sh = plan.shard(r);
	return launch_viewport(k, cam, d_rays, st, &sh, plan.n_rays(r));
}

// One frame on every device of a multi-device context.  render_shard(k, r, n, shard) enqueues device r's part on k->own_stream
// (n > 0 rays), leaving the RGBA8 pixels in k->rgba and, when out_accum is wanted, the float triples in k->accum; the tiles are
// then gathered to the first device, un-permuted there (k_assemble) and read back.
template <class RenderShard>
int multi_frame_impl(sphip_ctx* c, size_t w, size_t h, uint8_t* out_rgba, float* out_accum, const RenderShard& render_shard) {
	const int g = (int)c->kids.size();
	const RowPlan plan(w, h, g, (size_t)plan_tile_rows(h, g));
	const size_t pad = plan.max_rays(), npix = plan.npix;
	sphip_ctx* root = c->kids[0];
	HIP_TRY(c, hipSetDevice(root->device));
	int rc;
	if ((rc = ensure(c, c->gath, (size_t)g * pad * 4)) || (rc = ensure(c, c->img, npix * 4))) return rc;
	if (out_accum && ((rc = ensure(c, c->gath_acc, (size_t)g * pad * 12)) || (rc = ensure(c, c->img_acc, npix * 12)))) return rc;
	HIP_TRY(c, hipEventRecord(c->ev_g0, root->own_stream));
	const bool peer = c->gather_kind != SPHIP_GATHER_RCCL;
	std::vector<int> rcs((size_t)g, SPHIP_OK);
	std::vector<std::thread> th;
	for (int r = 0; r < g; ++r) th.emplace_back([&, r] {
		sphip_ctx* k = c->kids[(size_t)r];
		auto body = [&]() -> int {
			const size_t n = plan.n_rays(r);
			k->have_render = false;
			if (n == 0) return SPHIP_OK;
			HIP_TRY(k, hipSetDevice(k->device));
			int rc2;
			if ((rc2 = ensure(k, k->rgba, pad * 4))) return rc2;
			if (out_accum && (rc2 = ensure(k, k->accum, pad * 12))) return rc2;
			if ((rc2 = render_shard(k, r, n, plan.shard(r)))) return rc2;
			k->timed_upload = k->timed_download = false;
			return peer ? enqueue_peer_tile(c, k, r, n, pad, out_accum != nullptr) : SPHIP_OK;
		};
		rcs[(size_t)r] = body();
	});
	for (auto& t : th) t.join();
	for (int r = 0; r < g; ++r)
		if (rcs[(size_t)r]) return fail(c, rcs[(size_t)r], "device %d: %s", c->kids[(size_t)r]->device, c->kids[(size_t)r]->err.c_str());
	HIP_TRY(c, hipSetDevice(root->device));
	hipStream_t rs = root->own_stream;
	// peer-copy exchange, issued from this thread (the host threads do it themselves when peer copies are the context's exchange from the start)
	auto gather_peer_now = [&]() -> int {
		for (int r = 0; r < g; ++r) {
			if (!plan.n_rays(r)) continue;
			HIP_TRY(c, hipSetDevice(c->kids[(size_t)r]->device));
			if (const int rc2 = enqueue_peer_tile(c, c, r, plan.n_rays(r), pad, out_accum != nullptr)) return rc2;
		}
		HIP_TRY(c, hipSetDevice(root->device));
		return SPHIP_OK;
	};
	bool wait_tiles = peer;
	if (!peer) {
		// one grouped exchange: every other device sends its tiles, the first device receives them into its gather buffer;
		// its own tiles are a local copy
		if (plan.n_rays(0)) {
			HIP_TRY(c, hipMemcpyAsync(c->gath.p, root->rgba.p, plan.n_rays(0) * 4, hipMemcpyDeviceToDevice, rs));
			if (out_accum) HIP_TRY(c, hipMemcpyAsync(c->gath_acc.p, root->accum.p, plan.n_rays(0) * 12, hipMemcpyDeviceToDevice, rs));
		}
		int nrc = g_rccl.group_start();
		for (int r = 1; r < g && !nrc; ++r) {
			const size_t n = plan.n_rays(r);
			if (!n) continue;
			sphip_ctx* k = c->kids[(size_t)r];
			if (!nrc) nrc = g_rccl.send(k->rgba.p, n * 4, kNcclUint8, 0, c->comms[(size_t)r], k->own_stream);
			if (!nrc) nrc = g_rccl.recv((char*)c->gath.p + (size_t)r * pad * 4, n * 4, kNcclUint8, r, c->comms[0], rs);
			if (out_accum && !nrc) nrc = g_rccl.send(k->accum.p, n * 12, kNcclUint8, 0, c->comms[(size_t)r], k->own_stream);
			if (out_accum && !nrc) nrc = g_rccl.recv((char*)c->gath_acc.p + (size_t)r * pad * 12, n * 12, kNcclUint8, r, c->comms[0], rs);
		}
		const int erc = g_rccl.group_end();
		if (nrc || erc) {
			// the communicator did not take the exchange: this frame and every later one go through peer copies (the kernels'
			// results are still in each device's buffer); say so once, loudly
			fprintf(stderr, "libspath_hip: RCCL gather failed (%s); falling back to peer copies\n", g_rccl.errstr ? g_rccl.errstr(nrc ? nrc : erc) : "?");
			c->gather_kind = SPHIP_GATHER_PEER;
			if ((rc = gather_peer_now())) return rc;
			wait_tiles = true;
		}
	}
	if (wait_tiles)
		for (int r = 1; r < g; ++r) if (plan.n_rays(r)) HIP_TRY(c, hipStreamWaitEvent(rs, c->ev_tile[(size_t)r], 0));
	const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
	hipLaunchKernelGGL(sp::k_assemble<1>, grid, block, 0, rs, (const uint32_t*)c->gath.p, (uint32_t*)c->img.p, (uint32_t)npix, (uint32_t)plan.tile_px, (uint32_t)g, (uint32_t)pad);
	if (out_accum)
		hipLaunchKernelGGL(sp::k_assemble<3>, grid, block, 0, rs, (const uint32_t*)c->gath_acc.p, (uint32_t*)c->img_acc.p, (uint32_t)npix, (uint32_t)plan.tile_px, (uint32_t)g, (uint32_t)pad);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(c->ev_g1, rs));
	HIP_TRY(c, hipMemcpyAsync(out_rgba, c->img.p, npix * 4, hipMemcpyDeviceToHost, rs));
	if (out_accum) HIP_TRY(c, hipMemcpyAsync(out_accum, c->img_acc.p, npix * 12, hipMemcpyDeviceToHost, rs));
	HIP_TRY(c, hipStreamSynchronize(rs));            // blocking, like every reference backend (main.cpp:70-83)
	for (int r = 1; r < g; ++r) {                    // the other devices' streams are idle now too (their last work fed the gather)
		HIP_TRY(c, hipSetDevice(c->kids[(size_t)r]->device));
		HIP_TRY(c, hipStreamSynchronize(c->kids[(size_t)r]->own_stream));
	}
	c->have_render = true;
	c->stats.n_pixels = npix;
	c->stats.n_tris = c->n_tris;
	return SPHIP_OK;
}

// (on an error every device is drained: drain_all)
template <class RenderShard>
int multi_frame(sphip_ctx* c, size_t w, size_t h, uint8_t* out_rgba, float* out_accum, const RenderShard& render_shard) {
	const int rc = multi_frame_impl(c, w, h, out_rgba, out_accum, render_shard);
	if (rc != SPHIP_OK) drain_all(c);
	return rc;
}

// rays != nullptr: the caller's viewport (host array, w*h rays); else cam: every device generates the rays of its own tiles.
int multi_render(sphip_ctx* c, const float* rays, const sphip_camera* cam, size_t w, size_t h, size_t n_samples, uint64_t seed, int mode, int flags,
                 uint8_t* out_rgba, float* out_accum) {
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "render called before a scene was set");
	if (!out_rgba || w == 0 || h == 0 || w * h > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "bad render arguments (w=%zu h=%zu)", w, h);
	if (mode == SPHIP_MODE_PT && (n_samples == 0 || n_samples > 0x7fffffffull))
		return fail(c, SPHIP_E_INVALID, "n_samples must be in [1, 2^31) (the reference divides by it, cpu_renderer.cpp:77)");
	const RowPlan plan(w, h, (int)c->kids.size(), (size_t)plan_tile_rows(h, (int)c->kids.size()));
	sp::CamArgs ca{};
	if (cam) ca = cam_args_of(cam, c->lens);
	return multi_frame(c, w, h, out_rgba, out_accum, [&](sphip_ctx* k, int r, size_t n, const sphip_shard& sh) -> int {
		int rc2;
		if ((rc2 = ensure(k, k->rays, n * 24)) || (rc2 = deal_rays(k, plan, r, rays, cam, k->rays.p, k->own_stream))) return rc2;
		RenderCall call{ k->rays.p, n, n_samples, seed, mode, flags, k->rgba.p, out_accum ? k->accum.p : nullptr, k->own_stream };
		call.shard = &sh; call.cam = cam ? &ca : nullptr;
		return launch_render(k, call);
	});
}

// ---- adaptive sampling (sp_adaptive.h) on one device: a single-device context, or a child of a multi-device one for the n pixels
// of its shard.  Every pixel starts active, with count 0; the first list is every local pixel in order.
int adapt_begin_dev(sphip_ctx* k, size_t n, hipStream_t st) {
	int rc;
	const size_t nb = (n + 255) / 256;
	if ((rc = ensure(k, k->adp_s12, n * 16)) || (rc = ensure(k, k->adp_cnt, n * 4)) || (rc = ensure(k, k->adp_list[0], n * 4)) ||
	    (rc = ensure(k, k->adp_list[1], n * 4)) || (rc = ensure(k, k->adp_rays, n * 24)) || (rc = ensure(k, k->adp_keep, n)) ||
	    (rc = ensure(k, k->adp_blk, nb * 4)) || (rc = ensure(k, k->adp_nact_d, 4))) return rc;
	HIP_TRY(k, hipMemsetAsync(k->adp_cnt.p, 0, n * 4, st));
	hipLaunchKernelGGL(sp::k_adapt_iota, dim3((unsigned)nb), dim3(256), 0, st, (uint32_t*)k->adp_list[0].p, (uint32_t)n);
	HIP_TRY(k, hipGetLastError());
	k->adp_cur = 0;
	k->adp_nact = k->adp_nact_rb = (uint32_t)n;
	return SPHIP_OK;
}

// One adaptive step on device context k (par: the context holding the accumulation's parameters, k itself on a single device):
// the still-active pixels get global samples [total, total + n_samples), the rule and the compaction run on them, and the whole
// shard is resolved into k->rgba (and d_mean).  The new active count goes to k->adp_nact_rb in stream order.  With no active
// pixel nothing is traced: the resolve alone runs (same image), and the stats report 0 scans.
int adapt_step_dev(sphip_ctx* k, const sphip_ctx* par, size_t n, const sphip_shard& sh, size_t n_samples, float* d_mean, hipStream_t st) {
	const uint32_t na = k->adp_nact;
	int rc;
	if (na > 0) {
		const int cur = k->adp_cur;
		sp::AdaptArgs q{};
		q.sum = (float*)k->acc_sum.p;
		q.sample_base = (uint32_t)par->acc_total;
		q.list = (const uint32_t*)k->adp_list[cur].p;
		q.s12 = (double*)k->adp_s12.p;
		// every pixel active: the list is the identity, the gathered rays would be the accumulation's own
		const void* rays = na == n ? k->acc_rays.p : k->adp_rays.p;
		const sp::CamArgs ca = cam_args_of(&par->acc_cam, par->acc_lens);
		RenderCall call{ rays, na, n_samples, par->acc_seed, SPHIP_MODE_PT, par->acc_flags, k->rgba.p, nullptr, st };
		call.shard = &sh; call.adapt = &q; call.cam = par->acc_has_cam ? &ca : nullptr;
		if ((rc = launch_render(k, call))) return rc;
		const sp::AdaptRule rule{ par->adp_t, par->adp_floor, par->adp_min, (uint32_t)n_samples };
		const dim3 nb((unsigned)((na + 255) / 256));
		hipLaunchKernelGGL(sp::k_adapt_decide, nb, dim3(256), 0, st, q.list, na, (uint32_t*)k->adp_cnt.p, (const double*)q.s12, rule,
		                   (uint8_t*)k->adp_keep.p, (uint32_t*)k->adp_blk.p);
		hipLaunchKernelGGL(sp::k_adapt_scan, dim3(1), dim3(1024), 0, st, (uint32_t*)k->adp_blk.p, (uint32_t)nb.x, (uint32_t*)k->adp_nact_d.p);
		hipLaunchKernelGGL(sp::k_adapt_scatter, nb, dim3(256), 0, st, q.list, na, (const uint8_t*)k->adp_keep.p, (const uint32_t*)k->adp_blk.p,
		                   (const float*)k->acc_rays.p, (uint32_t*)k->adp_list[cur ^ 1].p, (float*)k->adp_rays.p);
		k->adp_cur = cur ^ 1;
		k->stats.n_launches += 4;
	} else {
		if ((rc = ensure(k, k->counter, 16 * sizeof(unsigned long long)))) return rc;
		HIP_TRY(k, hipMemsetAsync(k->counter.p, 0, 16 * sizeof(unsigned long long), st));
		HIP_TRY(k, hipEventRecord(k->ev_k0, st));
		k->stats.n_launches = 1;
		note_render(k, st, n, pick_variant(par->acc_flags, k->n_tris));
	}
	hipLaunchKernelGGL(sp::k_adapt_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)k->acc_sum.p,
	                   (const uint32_t*)k->adp_cnt.p, (uint32_t)n, (uint32_t*)k->rgba.p, d_mean);
	HIP_TRY(k, hipGetLastError());
	HIP_TRY(k, hipEventRecord(k->ev_k1, st));        // kernel_ms covers the path kernels, the rule, the compaction and the resolve
	if (na > 0) HIP_TRY(k, hipMemcpyAsync(&k->adp_nact_rb, k->adp_nact_d.p, 4, hipMemcpyDeviceToHost, st));
	else k->adp_nact_rb = 0;
	k->stats.n_pixels = n;
	return SPHIP_OK;
}

// sphip_accum_begin on a multi-device context: device r keeps the rays of its shard (the row-tile plan of the frame) and its
// shard's running sum resident
int multi_accum_begin(sphip_ctx* c, const float* rays, const sphip_camera* cam, size_t w, size_t h, bool adaptive) {
	const int g = (int)c->kids.size();
	const RowPlan plan(w, h, g, (size_t)plan_tile_rows(h, g));
	for (int r = 0; r < g; ++r) {
		sphip_ctx* k = c->kids[(size_t)r];
		const size_t n = plan.n_rays(r);
		k->adp_nact = k->adp_nact_rb = 0;
		if (n == 0) continue;
		auto body = [&]() -> int {
			HIP_TRY(k, hipSetDevice(k->device));
			int rc;
			if ((rc = ensure(k, k->acc_rays, n * 24)) || (rc = ensure(k, k->acc_sum, n * 12)) ||
			    (rc = deal_rays(k, plan, r, rays, cam, k->acc_rays.p, k->own_stream))) return rc;
			if (adaptive && (rc = adapt_begin_dev(k, n, k->own_stream))) return rc;
			HIP_TRY(k, hipStreamSynchronize(k->own_stream));       // the rays are borrowed
			return SPHIP_OK;
		};
		if (const int rc = body()) {
			drain_all(c);
			return fail(c, rc, "device %d: %s", k->device, k->err.c_str());
		}
	}
	return SPHIP_OK;
}

int multi_accum_step(sphip_ctx* c, size_t n_samples, uint8_t* out_rgba, float* out_mean) {
	if (c->adp_on) {                                  // every device runs the rule on its own row tiles
		const int rc = multi_frame(c, c->acc_w, c->acc_h, out_rgba, out_mean, [&](sphip_ctx* k, int, size_t n, const sphip_shard& sh) -> int {
			return adapt_step_dev(k, c, n, sh, n_samples, out_mean ? (float*)k->accum.p : nullptr, k->own_stream);
		});
		if (rc) return rc;
		uint64_t na = 0;                              // every stream has drained (multi_frame)
		for (sphip_ctx* k : c->kids) { k->adp_nact = k->adp_nact_rb; na += k->adp_nact; }
		c->adp_nact = (uint32_t)na;
		return SPHIP_OK;
	}
	const sp::CamArgs ca = cam_args_of(&c->acc_cam, c->acc_lens);
	return multi_frame(c, c->acc_w, c->acc_h, out_rgba, out_mean, [&](sphip_ctx* k, int, size_t n, const sphip_shard& sh) -> int {
		const sp::AccumArgs p{ (float*)k->acc_sum.p, (uint32_t)c->acc_total };
		RenderCall call{ k->acc_rays.p, n, n_samples, c->acc_seed, SPHIP_MODE_PT, c->acc_flags, k->rgba.p, out_mean ? k->accum.p : nullptr, k->own_stream };
		call.shard = &sh; call.prog = &p; call.cam = c->acc_has_cam ? &ca : nullptr;
		return launch_render(k, call);
	});
}

int multi_get_stats(sphip_ctx* c, sphip_stats* out) {
	if (!c->have_render) return fail(c, SPHIP_E_STATE, "no render has been issued yet");
	sphip_stats s{};
	s.kernel_ms_min = 1e300;
	for (sphip_ctx* k : c->kids) {
		if (!k->have_render) continue;
		sphip_stats ks;
		const int rc = sphip_get_stats(k, &ks);
		if (rc) return fail(c, rc, "device %d: %s", k->device, k->err.c_str());
		s.kernel_ms = std::max(s.kernel_ms, ks.kernel_ms);
		s.kernel_ms_min = std::min(s.kernel_ms_min, ks.kernel_ms);
		s.scans_executed += ks.scans_executed;
		s.kernel_variant = ks.kernel_variant;
		s.n_launches = ks.n_launches;
		++s.n_devices;
	}
	HIP_TRY(c, hipSetDevice(c->kids[0]->device));
	float ms = 0.0f;
	HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_g0, c->ev_g1));   // includes the first device's own kernels: report what is beyond them
	s.gather_ms = std::max(0.0, (double)ms - s.kernel_ms);
	s.gather_kind = (uint32_t)c->gather_kind;
	s.n_tris = c->n_tris;
	s.n_pixels = c->stats.n_pixels;
	c->stats = s;
	*out = s;
	return SPHIP_OK;
}

// sphip_accum_begin, and with adaptive != nullptr sphip_accum_begin_adaptive (the rule checked by the caller)
int accum_begin(sphip_t* c, const float* rays, const sphip_camera* cam, size_t w, size_t h, uint64_t seed, int flags, const sphip_adaptive* adaptive) {
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "sphip_accum_begin called before a scene was set");
	if ((rays == nullptr) == (cam == nullptr)) return fail(c, SPHIP_E_INVALID, "sphip_accum_begin takes exactly one of rays and cam");
	if (w == 0 || h == 0 || w * h > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "bad viewport size (w=%zu h=%zu)", w, h);
	if (cam && (cam->res_x != w || cam->res_y != h))
		return fail(c, SPHIP_E_INVALID, "w x h = %zux%zu differs from the camera's %ux%u", w, h, cam->res_x, cam->res_y);
	c->acc_on = false;                             // a begin that fails leaves no accumulation behind
	c->adp_on = false;
	c->acc_hist_on = false;
	c->dn_gbuf_ok = false;
	const int v = pick_variant(flags, c->n_tris);
	int rc;
	if ((rc = check_feature_rules(c, flags, v, SPHIP_MODE_PT, cam != nullptr))) return rc;
	if (!c->kids.empty()) {
		if ((rc = multi_accum_begin(c, rays, cam, w, h, adaptive != nullptr))) return rc;
	} else {
		HIP_TRY(c, hipSetDevice(c->device));
		const size_t n = w * h;
		hipStream_t st = c->own_stream;
		if ((rc = ensure(c, c->acc_rays, n * 24)) || (rc = ensure(c, c->acc_sum, n * 12))) return rc;
		if (rays) HIP_TRY(c, hipMemcpyAsync(c->acc_rays.p, rays, n * 24, hipMemcpyHostToDevice, st));      // once per accumulation
		else if ((rc = launch_viewport(c, cam, c->acc_rays.p, st))) return rc;
		if (adaptive && (rc = adapt_begin_dev(c, n, st))) return rc;
		HIP_TRY(c, hipStreamSynchronize(st));        // rays are borrowed
	}
	if (adaptive) {
		c->adp_on = true;
		c->adp_t = adaptive->rel_error; c->adp_floor = adaptive->floor; c->adp_min = adaptive->min_samples;
		c->adp_nact = (uint32_t)(w * h);
	}
	c->acc_on = true;
	c->acc_stale = false;
	c->acc_w = w; c->acc_h = h;
	c->acc_seed = seed; c->acc_flags = flags;
	c->acc_has_cam = cam != nullptr;               // the camera and the lens of camera samples, as they are at the begin
	if (cam) c->acc_cam = *cam;
	c->acc_lens = c->lens;
	c->acc_total = 0;                              // the first step's sample_base: the sum buffer's contents are not read
	return SPHIP_OK;
}

// =====================================================================================================================
// Denoising (sp_denoise.h; include/spath_hip.h: sphip_denoise): a G-buffer of the primary hits and an edge-aware a-trous
// filter, a post-process that leaves the scans, the sums and the raw image as they are.
// =====================================================================================================================

// the blend of sp_reproject.h for n pixels: the sum of `total` samples and a history (hist == nullptr: none) -> RGBA8 and mean (either may
// be nullptr).  after_render: the launch closes the kernel time of the render it follows.
int temporal_resolve_dev(sphip_ctx* c, size_t n, const void* sum, uint64_t total, const void* hmean, const void* hist, void* rgba, void* mean,
                         hipStream_t st, bool after_render) {
	const float inv_n = (float)(1.0 / (double)(total ? total : 1));    // as launch_render forms it
	hipLaunchKernelGGL(sp::k_temporal_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)sum, inv_n, (float)total,
	                   (const float*)hmean, (const float*)hist, (uint32_t)n, (uint32_t*)rgba, (float*)mean);
	HIP_TRY(c, hipGetLastError());
	if (after_render) {
		HIP_TRY(c, hipEventRecord(c->ev_k1, st));
		c->stats.n_launches += 1;
	}
	return SPHIP_OK;
}

int check_reproject(sphip_ctx* c, const sphip_reproject* P) {
	if (!P) return fail(c, SPHIP_E_INVALID, "null sphip_reproject");
	if (!std::isfinite(P->max_history) || P->max_history < 0.0f || !(P->normal_min >= -1.0f && P->normal_min <= 1.0f) ||
	    !std::isfinite(P->plane_tol) || P->plane_tol < 0.0f || P->reserved != 0)
		return fail(c, SPHIP_E_INVALID, "bad sphip_reproject {max_history %g, normal_min %g, plane_tol %g, reserved %u}: max_history and plane_tol "
		            "finite and >= 0, normal_min in [-1, 1], reserved 0", (double)P->max_history, (double)P->normal_min, (double)P->plane_tol, P->reserved);
	return SPHIP_OK;
}

// steps 1-6 of "temporal reprojection" (include/spath_hip.h) on device pointers; the arguments are checked by the callers
int reproject_dev(sphip_ctx* c, const sphip_reproject* P, const sphip_camera* prev, size_t w, size_t h, const void* rays_cur, const void* gbuf_cur,
                  const void* rays_prev, const void* gbuf_prev, const void* mean_prev, const void* hist_prev, void* out_mean, void* out_hist,
                  hipStream_t st) {
	const sp::ViewArgs v = view_args(prev);
	sp::ReprojArgs A{};
	A.rays_cur = (const float*)rays_cur; A.gbuf_cur = (const float4*)gbuf_cur;
	A.rays_prev = (const float*)rays_prev; A.gbuf_prev = (const float4*)gbuf_prev;
	A.mean_prev = (const float*)mean_prev; A.hist_prev = (const float*)hist_prev;
	A.out_mean = (float*)out_mean; A.out_hist = (float*)out_hist;
	A.w = (uint32_t)w; A.h = (uint32_t)h; A.n = (uint32_t)(w * h);
	A.px = v.px; A.py = v.py; A.pz = v.pz;
	A.cos_y = v.cos_y; A.sin_y = v.sin_y; A.cos_x = v.cos_x; A.sin_x = v.sin_x; A.focal = v.focal;
	A.xo = v.x_max - v.h_x_step; A.x_step = v.x_step;
	A.yo = v.y_max - v.h_y_step; A.y_step = v.y_step;
	A.max_history = P->max_history; A.normal_min = P->normal_min; A.plane_tol = P->plane_tol;
	hipLaunchKernelGGL(sp::k_reproject, dim3((unsigned)((w * h + 255) / 256)), dim3(256), 0, st, A);
	HIP_TRY(c, hipGetLastError());
	return SPHIP_OK;
}

int check_denoise(sphip_ctx* c, const sphip_denoise* P) {
	if (!P) return fail(c, SPHIP_E_INVALID, "null sphip_denoise");
	if (P->iterations > 8 || P->normal_log2 > 8 || !std::isfinite(P->sigma_depth) || !(P->sigma_depth > 0.0f) ||
	    !std::isfinite(P->sigma_lum) || !(P->sigma_lum > 0.0f) || P->reserved[0] || P->reserved[1])
		return fail(c, SPHIP_E_INVALID, "bad sphip_denoise {iterations %u, normal_log2 %u, sigma_depth %g, sigma_lum %g, reserved %u %u}: "
		            "iterations and normal_log2 in 0..8, sigmas finite and > 0, reserved 0", P->iterations, P->normal_log2,
		            (double)P->sigma_depth, (double)P->sigma_lum, P->reserved[0], P->reserved[1]);
	return SPHIP_OK;
}

// material class of every triangle: the smallest index whose 6 material floats are bitwise equal.  Derived on the host once per
// scene (the materials are read back: the one wait on the stream this path has)
int ensure_classes(sphip_ctx* c, hipStream_t st) {
	if (c->dn_cls_valid) return SPHIP_OK;
	const size_t n = c->n_tris;
	std::vector<uint32_t> m(n * 6);
	std::vector<int> cls(n);
	HIP_TRY(c, hipMemcpyAsync(m.data(), c->mats.p, n * 24, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	// triangle indices sorted by (material bits, index): in each run of equal materials the first is the smallest index
	std::vector<uint32_t> ord(n);
	for (size_t i = 0; i < n; ++i) ord[i] = (uint32_t)i;
	std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
		const int d = std::memcmp(&m[(size_t)a * 6], &m[(size_t)b * 6], 24);
		return d != 0 ? d < 0 : a < b;
	});
	for (size_t k = 0; k < n; ++k)
		cls[ord[k]] = (k > 0 && std::memcmp(&m[(size_t)ord[k] * 6], &m[(size_t)ord[k - 1] * 6], 24) == 0) ? cls[ord[k - 1]] : (int)ord[k];
	int rc;
	if ((rc = ensure(c, c->dn_cls, n * 4))) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->dn_cls.p, cls.data(), n * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipStreamSynchronize(st));             // cls is a local
	c->dn_cls_valid = true;
	return SPHIP_OK;
}

// G-buffer of n rays on a single-device context: the closest hits of sphip_closest_hit_device (same launch, same flags), then
// one entry per ray.  The stats describe both launches.
int gbuffer_dev(sphip_ctx* c, const void* d_rays, size_t n, int flags, void* d_out, hipStream_t st) {
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "G-buffer requested before a scene was set");
	if (!d_rays || !d_out) return fail(c, SPHIP_E_INVALID, "null ray or G-buffer pointer");
	if (n == 0 || n > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "n_rays %zu out of range", n);
	const bool smooth = (flags & SPHIP_FLAG_SMOOTH) != 0;  // the normals are the path's shading normals
	if (smooth && !c->have_vnorm) return fail(c, SPHIP_E_STATE, "SPHIP_FLAG_SMOOTH needs vertex normals (sphip_set_vertex_normals)");
	const bool nmap = (flags & SPHIP_FLAG_NORMAL_MAP) != 0;   // ... perturbed by the normal map
	if (nmap && !c->have_uv) return fail(c, SPHIP_E_STATE, "SPHIP_FLAG_NORMAL_MAP needs a UV table (sphip_set_uv)");
	if (nmap && !c->have_nmap) return fail(c, SPHIP_E_STATE, "SPHIP_FLAG_NORMAL_MAP needs a normal map (sphip_set_normal_map)");
	int rc;
	if (nmap && !smooth && (rc = ensure_zero_vnorm(c, st))) return rc;
	if ((rc = ensure_classes(c, st)) || (rc = ensure(c, c->dn_hit, n * 8))) return rc;
	int* idx = (int*)c->dn_hit.p;
	float* dist = (float*)((char*)c->dn_hit.p + n * 4);
	if ((rc = launch_render(c, RenderCall{ d_rays, n, 1, 0, kModeHits, flags, idx, dist, st }))) return rc;
	if (nmap) {
		sp::NmapArgs x{};
		x.uv = (const float*)c->uv.p; x.nmap = (const float*)c->nmap.p; x.nw = c->nmap_w; x.nh = c->nmap_h;
		hipLaunchKernelGGL(sp::k_gbuffer_nmap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)d_rays, (const int*)idx,
		                   (const float*)dist, (const float*)c->tris.p, (const float*)c->mats.p, (const int*)c->dn_cls.p, (uint32_t)n, (float4*)d_out,
		                   sp::NormArgs{ (const float*)(smooth ? c->vnorm.p : c->vnorm_zero.p) }, x);
	} else if (smooth)
		hipLaunchKernelGGL(sp::k_gbuffer_smooth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)d_rays, (const int*)idx,
		                   (const float*)dist, (const float*)c->tris.p, (const float*)c->mats.p, (const int*)c->dn_cls.p, (uint32_t)n, (float4*)d_out,
		                   sp::NormArgs{ (const float*)c->vnorm.p });
	else
		hipLaunchKernelGGL(sp::k_gbuffer, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)d_rays, (const int*)idx,
		                   (const float*)dist, (const float*)c->tris.p, (const float*)c->mats.p, (const int*)c->dn_cls.p, (uint32_t)n, (float4*)d_out);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(c->ev_k1, st));
	c->stats.n_launches += 1;
	return SPHIP_OK;
}

// the K iterations on the w*h float4 image in buffer a (written by the caller), ping-ponging with b (both of at least w*h*16 B,
// on c's device); the last one writes the outputs.  Adds the launches to *launches.
int atrous_run(sphip_ctx* c, const DevBuf& a, const DevBuf& b, const sphip_denoise* P, size_t w, size_t h, bool use_var, const void* gbuf,
               uint32_t* rgba, float* rgb, hipStream_t st, uint32_t* launches) {
	// SPATH_HIP_ATROUS=l2|lds picks the kernel for A/B runs (both give the same bytes); the default is the faster one measured
	// 
	const char* kenv = std::getenv("SPATH_HIP_ATROUS");
	const bool lds = !(kenv && std::strcmp(kenv, "l2") == 0);
	for (uint32_t i = 0; i < P->iterations; ++i) {
		const bool last = i + 1 == P->iterations;
		sp::AtrousArgs A{};
		A.in = (const float4*)(i % 2 ? b.p : a.p);
		A.out = (float4*)(i % 2 ? a.p : b.p);
		A.gbuf = (const float4*)gbuf;
		A.w = (uint32_t)w; A.h = (uint32_t)h;
		A.s = 1 << i;
		A.zs = P->sigma_depth * (float)A.s;
		A.sl2 = P->sigma_lum * P->sigma_lum;
		A.normal_log2 = P->normal_log2;
		A.use_var = use_var ? 1u : 0u;
		A.rgba = last ? rgba : nullptr;
		A.rgb = last ? rgb : nullptr;
		if (lds) {           // 16 x 16 blocks of each of the s x s sub-lattices
			const size_t su = (w + (size_t)A.s - 1) / (size_t)A.s, sv = (h + (size_t)A.s - 1) / (size_t)A.s;
			const dim3 grid((unsigned)((su + 15) / 16 * (size_t)A.s), (unsigned)((sv + 15) / 16 * (size_t)A.s));
			hipLaunchKernelGGL(sp::k_atrous_lds, grid, dim3(256), 0, st, A);
		} else {
			const dim3 grid((unsigned)((w + 15) / 16), (unsigned)((h + 15) / 16));
			hipLaunchKernelGGL(sp::k_atrous, grid, dim3(256), 0, st, A);
		}
	}
	HIP_TRY(c, hipGetLastError());
	*launches += P->iterations;
	return SPHIP_OK;
}

// start of a call's kernel time when no G-buffer is built: 0 scans
int dn_clock_start(sphip_ctx* c, hipStream_t st) {
	int rc;
	if ((rc = ensure(c, c->counter, 16 * sizeof(unsigned long long)))) return rc;
	HIP_TRY(c, hipMemsetAsync(c->counter.p, 0, 16 * sizeof(unsigned long long), st));
	HIP_TRY(c, hipEventRecord(c->ev_k0, st));
	c->stats.n_launches = 0;
	return SPHIP_OK;
}

// sphip_accum_denoise on a single-device context (k == c), or on the first device of a multi-device one with the frame's
// mean/variance (image order) already in c->dn_a.  d_rays: the frame's rays (for a G-buffer build).  Leaves the outputs in
// k->rgba / k->accum.  P == nullptr (sphip_accum_display without a filter): the mean itself, and no G-buffer is built or read.
// That path is this function's K = 0 form taken as it is, so that the display shows exactly the mean a filter would be given: it still
// writes the float4 pack into dn_a and a linear-clamp RGBA8 into k->rgba, neither of which the display tail reads (it overwrites
// k->rgba) -- about 20 B per pixel of stores beside the 12 B the tail needs, the price of one preparation of the mean instead of two.
int accum_denoise_dev(sphip_ctx* c, sphip_ctx* k, const sphip_denoise* P, const void* d_rays, bool have4, bool use_var, bool want_rgb,
                      hipStream_t st) {
	const size_t w = c->acc_w, h = c->acc_h, n = w * h;
	const sphip_denoise raw{};                         // K = 0: the input itself
	const bool filter = P != nullptr;
	if (!filter) P = &raw;
	int rc;
	if ((filter && (rc = ensure(c, c->dn_gbuf, n * 32))) || (rc = ensure(c, c->dn_a, n * 16)) || (rc = ensure(c, c->dn_b, n * 16)) ||
	    (rc = ensure(k, k->rgba, n * 4)) || (want_rgb && (rc = ensure(k, k->accum, n * 12)))) return rc;
	const bool build = filter && !c->dn_gbuf_ok;
	if (build) {
		if ((rc = gbuffer_dev(k, d_rays, n, c->acc_flags, c->dn_gbuf.p, st))) return rc;
	} else if ((rc = dn_clock_start(k, st))) return rc;
	uint32_t* rgba = (uint32_t*)k->rgba.p;
	float* rgb = want_rgb ? (float*)k->accum.p : nullptr;
	const bool k0 = P->iterations == 0;
	if (!have4 && c->acc_hist_on) {                    // a reprojected history (single-device, plain): the blended mean, no variance
		if ((rc = temporal_resolve_dev(k, n, c->acc_sum.p, c->acc_total, c->rp_hmean.p, c->rp_hist.p, nullptr, c->rp_pmean.p, st, false))) return rc;
		hipLaunchKernelGGL(sp::k_dn_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)c->rp_pmean.p, (const float*)nullptr,
		                   (uint32_t)n, (float4*)c->dn_a.p, k0 ? rgba : nullptr, k0 ? rgb : nullptr);
		k->stats.n_launches += 2;
	} else if (!have4) {
		hipLaunchKernelGGL(sp::k_dn_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)c->acc_sum.p,
		                   c->adp_on ? (const uint32_t*)c->adp_cnt.p : nullptr, (uint32_t)c->acc_total, c->adp_on ? (const double*)c->adp_s12.p : nullptr,
		                   (uint32_t)n, (float4*)c->dn_a.p, k0 ? rgba : nullptr, k0 ? rgb : nullptr);
		k->stats.n_launches += 1;
	} else if (k0) {
		hipLaunchKernelGGL(sp::k_dn_emit4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float4*)c->dn_a.p, (uint32_t)n, rgba, rgb);
		k->stats.n_launches += 1;
	}
	HIP_TRY(k, hipGetLastError());
	if ((rc = atrous_run(k, c->dn_a, c->dn_b, P, w, h, use_var, c->dn_gbuf.p, rgba, rgb, st, &k->stats.n_launches))) return rc;
	HIP_TRY(k, hipEventRecord(k->ev_k1, st));
	if (build) c->dn_gbuf_ok = true;
	note_render(k, st, n, pick_variant(c->acc_flags, k->n_tris));
	return SPHIP_OK;
}

// sphip_accum_denoise on a multi-device context: every device turns its shard's state into {mean, var}; the frame is put together in
// image order on the host (and, for a G-buffer build, the rays with it), uploaded to the first device and filtered there -- the
// per-pixel values do not depend on the sharding, so the bytes are those of a single-device context.  P == nullptr: the mean itself.
// post (sphip_accum_display): the display tail that follows on the first device, from root->accum (always written then) into root->rgba
// and, with out_rgb, root->dp_rgb
struct DisplayTail { const sphip_display* p; const sphip_metering* m; float* exposure_used; };
int display_tail(sphip_ctx* k, const sphip_display* p, const sphip_metering* m, size_t n, bool want_rgb, hipStream_t st, float* exposure_used);
int multi_accum_denoise(sphip_ctx* c, const sphip_denoise* P, uint8_t* out_rgba, float* out_rgb, const DisplayTail* post = nullptr) {
	const int g = (int)c->kids.size();
	const RowPlan plan(c->acc_w, c->acc_h, g, (size_t)plan_tile_rows(c->acc_h, g));
	const size_t npix = plan.npix;
	const bool need_rays = P != nullptr && !c->dn_gbuf_ok;
	sphip_ctx* root = c->kids[0];
	auto body = [&]() -> int {
		std::vector<float4> img4(npix);
		std::vector<float> rays(need_rays ? npix * 6 : 0);
		int rc;
		for (int r = 0; r < g; ++r) {
			sphip_ctx* k = c->kids[(size_t)r];
			k->have_render = false;
			const size_t n = plan.n_rays(r);
			if (n == 0) continue;
			HIP_TRY(c, hipSetDevice(k->device));
			if ((rc = ensure(k, k->dn_a, n * 16))) return fail(c, rc, "device %d: %s", k->device, k->err.c_str());
			hipLaunchKernelGGL(sp::k_dn_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const float*)k->acc_sum.p,
			                   c->adp_on ? (const uint32_t*)k->adp_cnt.p : nullptr, (uint32_t)c->acc_total, c->adp_on ? (const double*)k->adp_s12.p : nullptr,
			                   (uint32_t)n, (float4*)k->dn_a.p, (uint32_t*)nullptr, (float*)nullptr);
			HIP_TRY(c, hipGetLastError());
		}
		std::vector<ShardArray> arrays{ { &sphip_ctx::dn_a, 16, img4.data() } };
		if (need_rays) arrays.push_back({ &sphip_ctx::acc_rays, 24, rays.data() });
		if ((rc = read_shards(c, plan, arrays))) return rc;
		HIP_TRY(c, hipSetDevice(root->device));
		hipStream_t rs = root->own_stream;
		if ((rc = ensure(c, c->dn_a, npix * 16)) || (need_rays && (rc = ensure(c, c->dn_rays, npix * 24)))) return rc;
		HIP_TRY(c, hipEventRecord(c->ev_g0, rs));
		HIP_TRY(c, hipMemcpyAsync(c->dn_a.p, img4.data(), npix * 16, hipMemcpyHostToDevice, rs));
		if (need_rays) HIP_TRY(c, hipMemcpyAsync(c->dn_rays.p, rays.data(), npix * 24, hipMemcpyHostToDevice, rs));
		if ((rc = accum_denoise_dev(c, root, P, c->dn_rays.p, true, c->adp_on, out_rgb != nullptr || post != nullptr, rs)) ||
		    (post && (rc = display_tail(root, post->p, post->m, npix, out_rgb != nullptr, rs, post->exposure_used))))
			return fail(c, rc, "device %d: %s", root->device, root->err.c_str());
		HIP_TRY(c, hipEventRecord(c->ev_g1, rs));
		HIP_TRY(c, hipMemcpyAsync(out_rgba, root->rgba.p, npix * 4, hipMemcpyDeviceToHost, rs));
		if (out_rgb) HIP_TRY(c, hipMemcpyAsync(out_rgb, post ? root->dp_rgb.p : root->accum.p, npix * 12, hipMemcpyDeviceToHost, rs));
		HIP_TRY(c, hipStreamSynchronize(rs));          // img4 and rays are locals
		root->timed_upload = root->timed_download = false;
		c->have_render = true;
		c->stats.n_pixels = npix;
		c->stats.n_tris = c->n_tris;
		return SPHIP_OK;
	};
	const int rc = body();
	if (rc) drain_all(c);
	return rc;
}

// =====================================================================================================================
// Display transform (sp_display.h; include/spath_hip.h: sphip_display): metering by a luminance histogram, then exposure, a tone
// curve and the encoding in one pass over a mean image.  A post-process: it reads a mean and writes pixels, nothing else.
// =====================================================================================================================

const uint32_t kSrgbBits[255] = { SP_SRGB_THRESHOLD_BITS };

int check_display(sphip_ctx* c, const sphip_display* p) {
	if (!p) return fail(c, SPHIP_E_INVALID, "null sphip_display");
	if (!std::isfinite(p->exposure) || !(p->exposure > 0.0f) || !std::isfinite(p->white) || !(p->white > 0.0f) || p->curve > SPHIP_CURVE_FILMIC ||
	    p->encode > SPHIP_ENCODE_SRGB || p->reserved[0] || p->reserved[1])
		return fail(c, SPHIP_E_INVALID, "bad sphip_display {exposure %g, white %g, curve %u, encode %u, reserved %u %u}: exposure and white finite "
		            "and > 0, curve 0..2, encode 0..1, reserved 0", (double)p->exposure, (double)p->white, p->curve, p->encode, p->reserved[0], p->reserved[1]);
	return SPHIP_OK;
}

int check_metering(sphip_ctx* c, const sphip_metering* m) {
	if (!m) return fail(c, SPHIP_E_INVALID, "null sphip_metering");
	if (!std::isfinite(m->key) || !(m->key > 0.0f) || !(m->low >= 0.0f && m->low <= 1.0f) || !(m->high >= 0.0f && m->high <= 1.0f) ||
	    !(m->low < m->high) || m->reserved != 0)
		return fail(c, SPHIP_E_INVALID, "bad sphip_metering {key %g, low %g, high %g, reserved %u}: key finite and > 0, 0 <= low < high <= 1, "
		            "reserved 0", (double)m->key, (double)m->low, (double)m->high, m->reserved);
	return SPHIP_OK;
}

// "exposure from a histogram" of include/spath_hip.h: double, bins in ascending order, no libm beyond floor and ldexp (both exact)
float exposure_from_histogram(const uint32_t* hist, const sphip_metering* m) {
	uint64_t N = 0;
	for (uint32_t b = 8; b < 2040; ++b) N += hist[b];
	if (N == 0) return 1.0f;
	uint64_t lo = (uint64_t)((double)m->low * (double)N);
	uint64_t hi = N - (uint64_t)((1.0 - (double)m->high) * (double)N);
	if (hi <= lo) { lo = 0; hi = N; }
	uint64_t M = 0, cum = 0;
	double S = 0.0;
	for (uint32_t b = 8; b < 2040; ++b) {
		const uint64_t first = cum, last = cum + hist[b];          // the bin holds the ranks [first, last)
		cum = last;
		const uint64_t a = first > lo ? first : lo, z = last < hi ? last : hi;
		if (z <= a) continue;
		const uint64_t part = z - a;
		const double L = (double)((int)(b >> 3) - 127) + ((double)(b & 7u) + 0.5) / 8.0;
		M += part;
		S += (double)part * L;
	}
	const double mean = S / (double)M;
	double x = -mean;
	x = x < -126.0 ? -126.0 : (x > 126.0 ? 126.0 : x);
	const double f = std::floor(x);
	return (float)((double)m->key * std::ldexp(1.0 + (x - f), (int)f));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the histogram of n pixels of d_mean into d_hist (2048 u32, zeroed here on the same stream)
int histogram_dev(sphip_ctx* c, size_t n, const void* d_mean, void* d_hist, hipStream_t st) {
	HIP_TRY(c, hipMemsetAsync(d_hist, 0, sp::kLumBins * sizeof(uint32_t), st));
	const uint32_t nq = (uint32_t)(n / 4 + (n % 4 ? 1 : 0));
	const uint32_t blocks = std::min<uint32_t>((nq + 255u) / 256u, 2048u);
	hipLaunchKernelGGL(sp::k_lum_histogram, dim3(blocks), dim3(256), 0, st, (const float*)d_mean, (uint32_t)n, nq, aligned16(d_mean) ? 1u : 0u,
	                   (uint32_t*)d_hist);
	HIP_TRY(c, hipGetLastError());
	return SPHIP_OK;
}

// the transform of n pixels with the exposure given (p's own, or the metered one)
int display_dev(sphip_ctx* c, const sphip_display* p, float exposure, size_t n, const void* d_mean, void* d_rgba, void* d_rgb, hipStream_t st) {
	sp::DisplayArgs A{};
	A.mean = (const float*)d_mean; A.rgba = (uint32_t*)d_rgba; A.rgb = (float*)d_rgb;
	A.n = (uint32_t)n;
	A.exposure = exposure;
	A.w2 = p->white * p->white;
	A.curve = p->curve; A.encode = p->encode;
	A.vec = aligned16(d_mean) && aligned16(d_rgba) && aligned16(d_rgb) ? 1u : 0u;
	const size_t nq = n / 4 + (n % 4 ? 1 : 0);
	hipLaunchKernelGGL(sp::k_display, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, A);
	HIP_TRY(c, hipGetLastError());
	return SPHIP_OK;
}

// what sphip_accum_display does after the mean stands in k->accum (n pixels, k's device current): meter it (m != nullptr: one read-back
// of the 8 KB histogram), then the transform into k->rgba and, with want_rgb, k->dp_rgb.  Closes the call's kernel time.
int display_tail(sphip_ctx* k, const sphip_display* p, const sphip_metering* m, size_t n, bool want_rgb, hipStream_t st, float* exposure_used) {
	int rc;
	float E = p->exposure;
	if (m) {
		uint32_t hist[sp::kLumBins];
		if ((rc = ensure(k, k->dp_hist, sizeof hist)) || (rc = histogram_dev(k, n, k->accum.p, k->dp_hist.p, st))) return rc;
		HIP_TRY(k, hipMemcpyAsync(hist, k->dp_hist.p, sizeof hist, hipMemcpyDeviceToHost, st));
		HIP_TRY(k, hipStreamSynchronize(st));
		E = exposure_from_histogram(hist, m);
		k->stats.n_launches += 1;
	}
	if (want_rgb && (rc = ensure(k, k->dp_rgb, n * 12))) return rc;
	if ((rc = display_dev(k, p, E, n, k->accum.p, k->rgba.p, want_rgb ? k->dp_rgb.p : nullptr, st))) return rc;
	HIP_TRY(k, hipEventRecord(k->ev_k1, st));
	k->stats.n_launches += 1;
	*exposure_used = E;
	return SPHIP_OK;
}

} // namespace

extern "C" {

int sphip_abi_version(void) { return SPHIP_ABI_VERSION; }

const char* sphip_kernel_name(int variant) {
	if (variant < 0 || variant > kVariantLast) return nullptr;
	return kVariants[variant].name;
}

#ifndef SP_SOURCE_HASH
#define SP_SOURCE_HASH "unknown"
#endif
const char* sphip_build_info(void) { return "src=" SP_SOURCE_HASH; }

int sphip_kernel_available(int variant) { return variant_carried(variant) ? 1 : 0; }

int sphip_plan_tile_rows(size_t height, int n_devices) {
	if (height == 0 || n_devices < 1) return SPHIP_E_INVALID;
	return plan_tile_rows(height, n_devices);
}

int sphip_plan_shard(size_t width, size_t height, int n_devices, size_t tile_rows, int rank, sphip_shard* shard_out, size_t* n_rays_out) {
	if (width == 0 || height == 0 || n_devices < 1 || tile_rows == 0 || rank < 0 || rank >= n_devices) return SPHIP_E_INVALID;
	const RowPlan plan(width, height, n_devices, tile_rows);
	if (shard_out) *shard_out = plan.shard(rank);
	if (n_rays_out) *n_rays_out = plan.n_rays(rank);
	return SPHIP_OK;
}

int sphip_device_count(const sphip_t* c) { return c ? (c->kids.empty() ? 1 : (int)c->kids.size()) : 0; }

int sphip_create_multi(const int* device_ids, int n_devices, sphip_t** out) {
	if (!out) return fail(nullptr, SPHIP_E_INVALID, "out is NULL");
	*out = nullptr;
	std::vector<int> ids;
	if (device_ids) {
		if (n_devices < 1 || n_devices > 64) return fail(nullptr, SPHIP_E_INVALID, "n_devices %d out of range [1,64]", n_devices);
		ids.assign(device_ids, device_ids + n_devices);
	} else if (const char* env = getenv("SPATH_HIP_DEVICES")) {
		for (const char* p = env; *p;) {
			char* end = nullptr;
			const long v = strtol(p, &end, 10);
			if (end == p) return fail(nullptr, SPHIP_E_INVALID, "SPATH_HIP_DEVICES=\"%s\" is not a comma-separated list of device numbers", env);
			ids.push_back((int)v);
			p = (*end == ',') ? end + 1 : end;
			if (*end && *end != ',') return fail(nullptr, SPHIP_E_INVALID, "SPATH_HIP_DEVICES=\"%s\" is not a comma-separated list of device numbers", env);
		}
		if (ids.empty() || ids.size() > 64) return fail(nullptr, SPHIP_E_INVALID, "SPATH_HIP_DEVICES lists %zu devices", ids.size());
	} else {
		int n = 0;
		const hipError_t e = hipGetDeviceCount(&n);
		if (e != hipSuccess || n <= 0)
			return fail(nullptr, SPHIP_E_DEVICE, "no HIP device available (%s)", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
		for (int i = 0; i < n; ++i) ids.push_back(i);
	}
	const char* want = getenv("SPATH_HIP_GATHER");
	// one device: the plain context, no exchange step (unless the RCCL exchange is asked for explicitly: a communicator of one)
	if (ids.size() == 1 && !(want && !strcmp(want, "rccl"))) return sphip_create(ids[0], out);
	sphip_ctx* c = new (std::nothrow) sphip_ctx();
	if (!c) return fail(nullptr, SPHIP_E_DEVICE, "out of host memory");
	bool distinct = true;
	for (size_t i = 0; i < ids.size(); ++i) for (size_t j = 0; j < i; ++j) distinct &= ids[i] != ids[j];
	for (int id : ids) {
		sphip_ctx* k = nullptr;
		if (sphip_create(id, &k) != SPHIP_OK) { sphip_destroy(c); return SPHIP_E_DEVICE; }     // g_create_error already says why
		c->kids.push_back(k);
	}
	sphip_ctx* root = c->kids[0];
	c->device = root->device;
	hipError_t e = hipSetDevice(root->device);
	if (e == hipSuccess) e = hipEventCreate(&c->ev_g0);
	if (e == hipSuccess) e = hipEventCreate(&c->ev_g1);
	for (size_t r = 0; r < c->kids.size() && e == hipSuccess; ++r) {
		hipEvent_t ev = nullptr;
		if ((e = hipSetDevice(c->kids[r]->device)) == hipSuccess && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) == hipSuccess) c->ev_tile.push_back(ev);
		// direct xGMI copies into the first device's gather buffer (not an error if already enabled or unsupported: the copy still works, staged)
		if (e == hipSuccess && c->kids[r]->device != root->device) (void)hipDeviceEnablePeerAccess(root->device, 0);
		(void)hipGetLastError();
	}
	if (e != hipSuccess) { fail(nullptr, SPHIP_E_DEVICE, "multi-device init failed: %s", hipGetErrorString(e)); sphip_destroy(c); return SPHIP_E_DEVICE; }
	// exchange: RCCL when every listed device is a different GPU and librccl loads; peer copies otherwise
	c->gather_kind = SPHIP_GATHER_PEER;
	if (distinct && !(want && !strcmp(want, "peer"))) {
		c->rccl_lib = load_rccl();
		if (c->rccl_lib) {
			c->comms.assign(ids.size(), nullptr);
			const int nrc = g_rccl.init_all(c->comms.data(), (int)ids.size(), ids.data());
			if (nrc == 0) c->gather_kind = SPHIP_GATHER_RCCL;
			else { c->comms.clear(); if (want && !strcmp(want, "rccl")) { fail(nullptr, SPHIP_E_DEVICE, "ncclCommInitAll failed: %s", g_rccl.errstr ? g_rccl.errstr(nrc) : "?"); sphip_destroy(c); return SPHIP_E_DEVICE; } }
		} else if (want && !strcmp(want, "rccl")) { fail(nullptr, SPHIP_E_DEVICE, "SPATH_HIP_GATHER=rccl but librccl could not be loaded: %s", dlerror()); sphip_destroy(c); return SPHIP_E_DEVICE; }
	} else if (want && !strcmp(want, "rccl") && !distinct) {
		fail(nullptr, SPHIP_E_INVALID, "SPATH_HIP_GATHER=rccl needs distinct devices (a communicator holds a GPU once)"); sphip_destroy(c); return SPHIP_E_INVALID;
	}
	char d[320];
	snprintf(d, sizeof d, "HIP - Path Tracing (%zu devices, first: %s; pixel-row tiles, %s gather)", ids.size(),
	         root->desc.c_str() + (root->desc.rfind("(") == std::string::npos ? 0 : root->desc.rfind("(") + 1), c->gather_kind == SPHIP_GATHER_RCCL ? "RCCL" : "peer-copy");
	c->desc = d;
	*out = c;
	return SPHIP_OK;
}

int sphip_create(int device_id, sphip_t** out) {
	if (!out) return fail(nullptr, SPHIP_E_INVALID, "out is NULL");
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0)
		return fail(nullptr, SPHIP_E_DEVICE, "no HIP device available (%s)", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
	if (device_id < 0 || device_id >= n) return fail(nullptr, SPHIP_E_INVALID, "device %d out of range [0,%d)", device_id, n);
	sphip_ctx* c = new (std::nothrow) sphip_ctx();
	if (!c) return fail(nullptr, SPHIP_E_DEVICE, "out of host memory");
	c->device = device_id;
	hipDeviceProp_t prop;
	if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess ||
	    (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
		fail(nullptr, SPHIP_E_DEVICE, "device %d init failed: %s", device_id, hipGetErrorString(e));
		delete c;
		return SPHIP_E_DEVICE;
	}
	hipEvent_t* evs[6] = { &c->ev_k0, &c->ev_k1, &c->ev_u0, &c->ev_u1, &c->ev_d0, &c->ev_d1 };
	for (auto ev : evs) {
		if ((e = hipEventCreate(ev)) != hipSuccess) {
			fail(nullptr, SPHIP_E_DEVICE, "hipEventCreate failed: %s", hipGetErrorString(e));
			sphip_destroy(c);
			return SPHIP_E_DEVICE;
		}
	}
	char d[256];
	snprintf(d, sizeof d, "HIP - Path Tracing (%s, %s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
	c->desc = d;
	*out = c;
	return SPHIP_OK;
}

void sphip_destroy(sphip_t* c) {
	if (!c) return;
	if (!c->kids.empty()) {
		for (void* comm : c->comms) if (comm) (void)g_rccl.destroy(comm);
		const int dev = c->kids[0]->device;            // the parent's buffers live there
		(void)hipSetDevice(dev);
		(void)hipDeviceSynchronize();
		if (c->ev_g0) (void)hipEventDestroy(c->ev_g0);
		if (c->ev_g1) (void)hipEventDestroy(c->ev_g1);
		for (size_t r = 0; r < c->ev_tile.size(); ++r) { (void)hipSetDevice(c->kids[r]->device); (void)hipEventDestroy(c->ev_tile[r]); }
		for (sphip_ctx* k : c->kids) sphip_destroy(k);
		(void)hipSetDevice(dev);
		delete c;                                      // every DevBuf frees itself
		return;
	}
	(void)hipSetDevice(c->device);
	if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
	hipEvent_t evs[6] = { c->ev_k0, c->ev_k1, c->ev_u0, c->ev_u1, c->ev_d0, c->ev_d1 };
	for (auto ev : evs) if (ev) (void)hipEventDestroy(ev);
	if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
	delete c;
}

const char* sphip_last_error(const sphip_t* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

const char* sphip_description(const sphip_t* c) { return c ? c->desc.c_str() : "HIP - Path Tracing"; }

int sphip_set_scene(sphip_t* c, const float* tris, const float* mats, size_t n_tris) {
	if (!c) return SPHIP_E_INVALID;
	if (!tris || !mats || n_tris == 0 || n_tris > 0x7fffffffull) return fail(c, SPHIP_E_INVALID, "bad scene arguments (n_tris=%zu)", n_tris);
	c->acc_stale = c->acc_on;                      // the running sum belongs to the old scene
	c->dn_cls_valid = false;
	if (!c->kids.empty()) return multi_set_scene(c, tris, mats, n_tris);
	HIP_TRY(c, hipSetDevice(c->device));
	int rc;
	if ((rc = ensure(c, c->tris, n_tris * 48)) || (rc = ensure(c, c->mats, n_tris * 24))) return rc;
	c->n_tris = n_tris;
	HIP_TRY(c, hipMemcpyAsync(c->tris.p, tris, n_tris * 48, hipMemcpyHostToDevice, c->own_stream));
	HIP_TRY(c, hipMemcpyAsync(c->mats.p, mats, n_tris * 24, hipMemcpyHostToDevice, c->own_stream));
	if ((rc = repack(c, c->own_stream))) return rc;
	HIP_TRY(c, hipStreamSynchronize(c->own_stream));   // tris/mats are borrowed: do not outlive the call
	return SPHIP_OK;
}

int sphip_set_scene_device(sphip_t* c, const void* d_tris, const void* d_mats, size_t n_tris, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	if (!d_tris || !d_mats || n_tris == 0 || n_tris > 0x7fffffffull) return fail(c, SPHIP_E_INVALID, "bad scene arguments (n_tris=%zu)", n_tris);
	c->acc_stale = c->acc_on;
	c->dn_cls_valid = false;
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = (hipStream_t)stream;
	int rc;
	if ((rc = ensure(c, c->tris, n_tris * 48)) || (rc = ensure(c, c->mats, n_tris * 24))) return rc;
	c->n_tris = n_tris;
	HIP_TRY(c, hipMemcpyAsync(c->tris.p, d_tris, n_tris * 48, hipMemcpyDeviceToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(c->mats.p, d_mats, n_tris * 24, hipMemcpyDeviceToDevice, st));
	return repack(c, st);
}

// the per-triangle tables: kTriTables (sp_host_tables.h) says what differs between them, set_table and set_table_device do the work
int sphip_set_specular(sphip_t* c, const float* spec) { return set_table(c, kTabSpecular, spec); }
int sphip_set_specular_device(sphip_t* c, const void* d_spec, void* stream) { return set_table_device(c, kTabSpecular, d_spec, stream); }
int sphip_set_vertex_normals(sphip_t* c, const float* vn) { return set_table(c, kTabVertexNormals, vn); }
int sphip_set_vertex_normals_device(sphip_t* c, const void* d_vn, void* stream) { return set_table_device(c, kTabVertexNormals, d_vn, stream); }
int sphip_set_dielectric(sphip_t* c, const float* glass) { return set_table(c, kTabDielectric, glass); }
int sphip_set_dielectric_device(sphip_t* c, const void* d_glass, void* stream) { return set_table_device(c, kTabDielectric, d_glass, stream); }
int sphip_set_roughness(sphip_t* c, const float* alpha) { return set_table(c, kTabRoughness, alpha); }
int sphip_set_roughness_device(sphip_t* c, const void* d_alpha, void* stream) { return set_table_device(c, kTabRoughness, d_alpha, stream); }
int sphip_set_uv(sphip_t* c, const float* uv) { return set_table(c, kTabUv, uv); }
int sphip_set_uv_device(sphip_t* c, const void* d_uv, void* stream) { return set_table_device(c, kTabUv, d_uv, stream); }

// the texels of a host-pointer image, w x h x {r g b}: every value finite and >= 0
static int check_texels(sphip_ctx* c, const char* noun, const float* texels, uint32_t w, uint32_t h) {
	const size_t count = (size_t)w * h * 3, bad = first_bad_texel(texels, count);
	return bad < count ? fail(c, SPHIP_E_INVALID, "%s", bad_texel_message(noun, texels, bad, w).c_str()) : SPHIP_OK;
}

int sphip_set_environment(sphip_t* c, const float* texels, uint32_t n) {
	if (!c) return SPHIP_E_INVALID;
	if (texels) {
		if (n == 0 || n > sp::kEnvMaxN) return fail(c, SPHIP_E_INVALID, "environment map: n = %u (1 <= n <= %u)", n, sp::kEnvMaxN);
		if (const int rc = check_texels(c, "environment map", texels, n, n)) return rc;
	}
	if (c->kids.empty()) return set_env_map(c, texels, n, hipMemcpyHostToDevice, c->own_stream, true);
	if (const int rc = set_on_every_device(c, &sphip_ctx::have_env, texels != nullptr,        // the texels were validated above, once
	                                       [&](sphip_ctx* k) { return set_env_map(k, texels, n, hipMemcpyHostToDevice, k->own_stream, true); })) return rc;
	c->env_n = texels ? n : 0;
	return SPHIP_OK;
}

int sphip_set_environment_device(sphip_t* c, const void* d_texels, uint32_t n, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	const bool bad = d_texels && (n == 0 || n > sp::kEnvMaxN);        // refused, and like every call it leaves no map behind
	const int rc = set_env_map(c, bad ? nullptr : d_texels, n, hipMemcpyDeviceToDevice, (hipStream_t)stream, false);
	return bad ? fail(c, SPHIP_E_INVALID, "environment map: n = %u (1 <= n <= %u)", n, sp::kEnvMaxN) : rc;
}

// the atlas of a single-device context from src (tw * th * 3 f32), or no atlas with src == nullptr; sync: src is borrowed host memory
static int set_atlas(sphip_ctx* c, const void* src, uint32_t tw, uint32_t th, hipMemcpyKind kind, hipStream_t st, bool sync) {
	c->acc_stale = c->acc_on;                      // the running sum was rendered under the old atlas
	c->have_tex = false;
	if (!src) return SPHIP_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	const size_t bytes = (size_t)tw * th * 12;
	if (const int rc = ensure(c, c->atlas, bytes)) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->atlas.p, src, bytes, kind, st));
	if (sync) HIP_TRY(c, hipStreamSynchronize(st));
	c->tex_w = tw; c->tex_h = th;
	c->have_tex = true;
	return SPHIP_OK;
}

int sphip_set_texture(sphip_t* c, const float* texels, uint32_t tw, uint32_t th) {
	if (!c) return SPHIP_E_INVALID;
	if (texels) {
		if (tw == 0 || tw > sp::kTexMaxN || th == 0 || th > sp::kTexMaxN)
			return fail(c, SPHIP_E_INVALID, "atlas: %u x %u texels (1 <= tw, th <= %u)", tw, th, sp::kTexMaxN);
		if (const int rc = check_texels(c, "atlas", texels, tw, th)) return rc;
	}
	if (c->kids.empty()) return set_atlas(c, texels, tw, th, hipMemcpyHostToDevice, c->own_stream, true);
	if (const int rc = set_on_every_device(c, &sphip_ctx::have_tex, texels != nullptr,        // the texels were validated above, once
	                                       [&](sphip_ctx* k) { return set_atlas(k, texels, tw, th, hipMemcpyHostToDevice, k->own_stream, true); })) return rc;
	c->tex_w = texels ? tw : 0; c->tex_h = texels ? th : 0;
	return SPHIP_OK;
}

int sphip_set_texture_device(sphip_t* c, const void* d_texels, uint32_t tw, uint32_t th, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	const bool bad = d_texels && (tw == 0 || tw > sp::kTexMaxN || th == 0 || th > sp::kTexMaxN);   // refused, and like every call it leaves no atlas behind
	const int rc = set_atlas(c, bad ? nullptr : d_texels, tw, th, hipMemcpyDeviceToDevice, (hipStream_t)stream, false);
	return bad ? fail(c, SPHIP_E_INVALID, "atlas: %u x %u texels (1 <= tw, th <= %u)", tw, th, sp::kTexMaxN) : rc;
}

// the normal map of a single-device context from src (nw * nh * 3 f32), or no map with src == nullptr; sync: src is borrowed host memory
static int set_nmap(sphip_ctx* c, const void* src, uint32_t nw, uint32_t nh, hipMemcpyKind kind, hipStream_t st, bool sync) {
	c->acc_stale = c->acc_on;                      // the running sum was rendered under the old map
	c->have_nmap = false;
	if (!src) return SPHIP_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	const size_t bytes = (size_t)nw * nh * 12;
	if (const int rc = ensure(c, c->nmap, bytes)) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->nmap.p, src, bytes, kind, st));
	if (sync) HIP_TRY(c, hipStreamSynchronize(st));
	c->nmap_w = nw; c->nmap_h = nh;
	c->have_nmap = true;
	return SPHIP_OK;
}

int sphip_set_normal_map(sphip_t* c, const float* texels, uint32_t nw, uint32_t nh) {
	if (!c) return SPHIP_E_INVALID;
	if (texels) {
		if (nw == 0 || nw > sp::kTexMaxN || nh == 0 || nh > sp::kTexMaxN)
			return fail(c, SPHIP_E_INVALID, "normal map: %u x %u texels (1 <= nw, nh <= %u)", nw, nh, sp::kTexMaxN);
		const size_t count = (size_t)nw * nh * 3, bad = first_nonfinite_texel(texels, count);    // negative values are legal here
		if (bad < count) return fail(c, SPHIP_E_INVALID, "%s", nonfinite_texel_message("normal map", texels, bad, nw).c_str());
	}
	if (c->kids.empty()) return set_nmap(c, texels, nw, nh, hipMemcpyHostToDevice, c->own_stream, true);
	if (const int rc = set_on_every_device(c, &sphip_ctx::have_nmap, texels != nullptr,       // the texels were validated above, once
	                                       [&](sphip_ctx* k) { return set_nmap(k, texels, nw, nh, hipMemcpyHostToDevice, k->own_stream, true); })) return rc;
	c->nmap_w = texels ? nw : 0; c->nmap_h = texels ? nh : 0;
	return SPHIP_OK;
}

int sphip_set_normal_map_device(sphip_t* c, const void* d_texels, uint32_t nw, uint32_t nh, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	const bool bad = d_texels && (nw == 0 || nw > sp::kTexMaxN || nh == 0 || nh > sp::kTexMaxN);   // refused, and like every call it leaves no map behind
	const int rc = set_nmap(c, bad ? nullptr : d_texels, nw, nh, hipMemcpyDeviceToDevice, (hipStream_t)stream, false);
	return bad ? fail(c, SPHIP_E_INVALID, "normal map: %u x %u texels (1 <= nw, nh <= %u)", nw, nh, sp::kTexMaxN) : rc;
}

int sphip_render_device(sphip_t* c, const void* d_rays, size_t n_rays, const sphip_shard* shard, size_t image_width,
                        size_t n_samples, uint64_t seed, int mode, int flags, void* d_out_rgba, void* d_out_accum, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	HIP_TRY(c, hipSetDevice(c->device));
	c->timed_upload = c->timed_download = false;
	RenderCall call{ d_rays, n_rays, n_samples, seed, mode, flags, d_out_rgba, d_out_accum, (hipStream_t)stream };
	call.shard = shard;
	return launch_render(c, call);
}

int sphip_render_device_accum(sphip_t* c, const void* d_rays, size_t n_rays, const sphip_shard* shard, size_t image_width,
                              uint64_t sample_base, size_t n_samples, uint64_t seed, int flags, void* d_sum,
                              void* d_out_rgba, void* d_out_mean, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	if (!d_sum) return fail(c, SPHIP_E_INVALID, "null sum pointer");
	if (sample_base > 0x7fffffffull) return fail(c, SPHIP_E_INVALID, "sample_base %llu: the total must stay below 2^31", (unsigned long long)sample_base);
	HIP_TRY(c, hipSetDevice(c->device));
	c->timed_upload = c->timed_download = false;
	const sp::AccumArgs p{ (float*)d_sum, (uint32_t)sample_base };
	RenderCall call{ d_rays, n_rays, n_samples, seed, SPHIP_MODE_PT, flags, d_out_rgba, d_out_mean, (hipStream_t)stream };
	call.shard = shard; call.prog = &p;
	return launch_render(c, call);
}


int sphip_accum_begin(sphip_t* c, const float* rays, const sphip_camera* cam, size_t w, size_t h, uint64_t seed, int flags) {
	if (!c) return SPHIP_E_INVALID;
	return accum_begin(c, rays, cam, w, h, seed, flags, nullptr);
}

int sphip_accum_begin_adaptive(sphip_t* c, const float* rays, const sphip_camera* cam, size_t w, size_t h, uint64_t seed, int flags,
                               const sphip_adaptive* a) {
	if (!c) return SPHIP_E_INVALID;
	if (!a) return fail(c, SPHIP_E_INVALID, "null sphip_adaptive");
	if (!std::isfinite(a->rel_error) || a->rel_error < 0.0 || !std::isfinite(a->floor) || a->floor < 0.0 || a->min_samples < 2 || a->reserved != 0)
		return fail(c, SPHIP_E_INVALID, "bad sphip_adaptive {rel_error %g, floor %g, min_samples %u, reserved %u}: t and floor finite and >= 0, "
		            "min_samples >= 2, reserved 0", a->rel_error, a->floor, a->min_samples, a->reserved);
	return accum_begin(c, rays, cam, w, h, seed, flags, a);
}

int sphip_accum_counts(sphip_t* c, uint32_t* out_counts, uint64_t* n_active_out) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->acc_on) return fail(c, SPHIP_E_STATE, "sphip_accum_counts called with no accumulation begun");
	const size_t npix = c->acc_w * c->acc_h;
	if (n_active_out) *n_active_out = c->adp_on ? c->adp_nact : npix;
	if (!out_counts) return SPHIP_OK;
	if (!c->adp_on) {
		std::fill(out_counts, out_counts + npix, (uint32_t)c->acc_total);
		return SPHIP_OK;
	}
	if (c->kids.empty()) {
		HIP_TRY(c, hipSetDevice(c->device));
		HIP_TRY(c, hipMemcpyAsync(out_counts, c->adp_cnt.p, npix * 4, hipMemcpyDeviceToHost, c->own_stream));
		HIP_TRY(c, hipStreamSynchronize(c->own_stream));
		return SPHIP_OK;
	}
	// each device's counts in its shard's order, put in image order
	const int g = (int)c->kids.size();
	const RowPlan plan(c->acc_w, c->acc_h, g, (size_t)plan_tile_rows(c->acc_h, g));
	return read_shards(c, plan, { { &sphip_ctx::adp_cnt, 4, out_counts } });
}

int sphip_accum_step(sphip_t* c, size_t n_samples, uint8_t* out_rgba, float* out_mean, uint64_t* total_out) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->acc_on) return fail(c, SPHIP_E_STATE, "sphip_accum_step called with no accumulation begun (sphip_accum_begin)");
	if (c->acc_stale) return fail(c, SPHIP_E_STATE, "the scene changed since sphip_accum_begin: begin a new accumulation");
	if (!out_rgba) return fail(c, SPHIP_E_INVALID, "null output pointer");
	if (n_samples == 0 || c->acc_total + n_samples > 0x7fffffffull)
		return fail(c, SPHIP_E_INVALID, "n_samples = %zu after %llu: each step renders at least one sample, and the total must stay below 2^31",
		            n_samples, (unsigned long long)c->acc_total);
	const bool traced = !c->adp_on || c->adp_nact > 0;   // an adaptive step with no active pixel renders nothing
	int rc;
	if (!c->kids.empty()) {
		rc = multi_accum_step(c, n_samples, out_rgba, out_mean);
	} else {
		auto body = [&]() -> int {
			HIP_TRY(c, hipSetDevice(c->device));
			const size_t n = c->acc_w * c->acc_h;
			hipStream_t st = c->own_stream;
			int rc2;
			if ((rc2 = ensure(c, c->rgba, n * 4))) return rc2;
			if (out_mean && (rc2 = ensure(c, c->accum, n * 12))) return rc2;
			const sp::AccumArgs p{ (float*)c->acc_sum.p, (uint32_t)c->acc_total };
			const sphip_shard whole{ 0, n, 0 };
			if (c->adp_on) {
				if ((rc2 = adapt_step_dev(c, c, n, whole, n_samples, out_mean ? (float*)c->accum.p : nullptr, st))) return rc2;
			} else {
				const sp::CamArgs ca = cam_args_of(&c->acc_cam, c->acc_lens);
				RenderCall call{ c->acc_rays.p, n, n_samples, c->acc_seed, SPHIP_MODE_PT, c->acc_flags, c->rgba.p, out_mean ? c->accum.p : nullptr, st };
				call.prog = &p; call.cam = c->acc_has_cam ? &ca : nullptr;
				if ((rc2 = launch_render(c, call))) return rc2;
				// a reprojected history: the frame is the blend of it with the sum (sp_reproject.h); pixels without one keep their bits
				if (c->acc_hist_on && (rc2 = temporal_resolve_dev(c, n, c->acc_sum.p, c->acc_total + n_samples, c->rp_hmean.p, c->rp_hist.p,
				                                                  c->rgba.p, out_mean ? c->accum.p : nullptr, st, true))) return rc2;
			}
			if ((rc2 = download_frame(c, n, out_rgba, out_mean, st))) return rc2;
			c->adp_nact = c->adp_nact_rb;
			c->timed_upload = false;
			c->timed_download = true;
			return SPHIP_OK;
		};
		rc = body();
		if (rc) { (void)hipStreamSynchronize(c->own_stream); (void)hipGetLastError(); }
	}
	if (rc) {                                      // the sums may hold part of this step: nothing can continue from them
		c->acc_on = false;
		return rc;
	}
	if (traced) c->acc_total += n_samples;
	if (total_out) *total_out = c->acc_total;
	return SPHIP_OK;
}

int sphip_viewport_device(sphip_t* c, const sphip_camera* cam, void* d_rays_out, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	HIP_TRY(c, hipSetDevice(c->device));
	return launch_viewport(c, cam, d_rays_out, (hipStream_t)stream);
}

int sphip_set_lens(sphip_t* c, const sphip_lens* lens) {
	if (!c) return SPHIP_E_INVALID;
	const sphip_lens l = lens ? *lens : sphip_lens{ 0.0f, 0.0f, 0 };
	if (!std::isfinite(l.aperture) || l.aperture < 0.0f || (l.aperture > 0.0f && !(std::isfinite(l.focus_dist) && l.focus_dist > 0.0f)) || l.reserved != 0)
		return fail(c, SPHIP_E_INVALID, "bad sphip_lens {aperture %g, focus_dist %g, reserved %u}: aperture finite and >= 0, focus_dist finite and > 0 "
		            "when aperture > 0, reserved 0", (double)l.aperture, (double)l.focus_dist, l.reserved);
	c->lens = l;
	return SPHIP_OK;
}

int sphip_camera_rays_device(sphip_t* c, const sphip_camera* cam, uint64_t seed, uint32_t sample, void* d_rays_out, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	if (!cam || !d_rays_out) return fail(c, SPHIP_E_INVALID, "null camera or ray pointer");
	if (cam->res_x == 0 || cam->res_y == 0 || (uint64_t)cam->res_x * cam->res_y > 0xffffffffull)
		return fail(c, SPHIP_E_INVALID, "bad viewport size %ux%u", cam->res_x, cam->res_y);
	HIP_TRY(c, hipSetDevice(c->device));
	const sp::CamArgs ca = cam_args_of(cam, c->lens);
	hipLaunchKernelGGL(sp::k_camera_rays, dim3((ca.v.n_local + 255) / 256), dim3(256), 0, (hipStream_t)stream, ca, seed, sample, (float*)d_rays_out);
	HIP_TRY(c, hipGetLastError());
	return SPHIP_OK;
}

int sphip_render_camera(sphip_t* c, const sphip_camera* cam, size_t n_samples, uint64_t seed, int mode, int flags,
                        uint8_t* out_rgba, float* out_accum) {
	if (!c) return SPHIP_E_INVALID;
	if (!cam || !out_rgba) return fail(c, SPHIP_E_INVALID, "null camera or output pointer");
	if (!c->kids.empty()) return multi_render(c, nullptr, cam, cam->res_x, cam->res_y, n_samples, seed, mode, flags, out_rgba, out_accum);
	HIP_TRY(c, hipSetDevice(c->device));
	const size_t n = (size_t)cam->res_x * cam->res_y;
	hipStream_t st = c->own_stream;
	int rc;
	if ((rc = ensure(c, c->rays, (n ? n : 1) * 24)) || (rc = ensure(c, c->rgba, (n ? n : 1) * 4))) return rc;
	if (out_accum && (rc = ensure(c, c->accum, n * 12))) return rc;
	if ((rc = launch_viewport(c, cam, c->rays.p, st))) return rc;
	const sp::CamArgs ca = cam_args_of(cam, c->lens);
	RenderCall call{ c->rays.p, n, n_samples, seed, mode, flags, c->rgba.p, out_accum ? c->accum.p : nullptr, st };
	call.cam = &ca;
	if ((rc = launch_render(c, call))) return rc;
	if ((rc = download_frame(c, n, out_rgba, out_accum, st))) return rc;
	c->timed_upload = false;
	c->timed_download = true;
	return SPHIP_OK;
}

int sphip_closest_hit_device(sphip_t* c, const void* d_rays, size_t n_rays, const void* d_src_idx, int flags,
                             void* d_out_idx, void* d_out_dist, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	HIP_TRY(c, hipSetDevice(c->device));
	c->timed_upload = c->timed_download = false;
	RenderCall call{ d_rays, n_rays, 1, 0, kModeHits, flags, d_out_idx, d_out_dist, (hipStream_t)stream };
	call.src = (const int*)d_src_idx;
	return launch_render(c, call);
}

int sphip_render(sphip_t* c, const float* rays, size_t w, size_t h, size_t n_samples, uint64_t seed, int mode, int flags,
                 uint8_t* out_rgba, float* out_accum) {
	if (!c) return SPHIP_E_INVALID;
	if (!rays || !out_rgba || w == 0 || h == 0) return fail(c, SPHIP_E_INVALID, "bad render arguments (w=%zu h=%zu)", w, h);
	if (!c->kids.empty()) return multi_render(c, rays, nullptr, w, h, n_samples, seed, mode, flags, out_rgba, out_accum);
	HIP_TRY(c, hipSetDevice(c->device));
	const size_t n = w * h;
	hipStream_t st = c->own_stream;
	int rc;
	if ((rc = ensure(c, c->rays, n * 24)) || (rc = ensure(c, c->rgba, n * 4))) return rc;
	if (out_accum && (rc = ensure(c, c->accum, n * 12))) return rc;
	HIP_TRY(c, hipEventRecord(c->ev_u0, st));
	HIP_TRY(c, hipMemcpyAsync(c->rays.p, rays, n * 24, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipEventRecord(c->ev_u1, st));
	if ((rc = launch_render(c, RenderCall{ c->rays.p, n, n_samples, seed, mode, flags, c->rgba.p, out_accum ? c->accum.p : nullptr, st }))) return rc;
	if ((rc = download_frame(c, n, out_rgba, out_accum, st))) return rc;
	c->timed_upload = c->timed_download = true;
	return SPHIP_OK;
}

int sphip_selftest_device(sphip_t* c, int what, const void* in, size_t n, void* out) {
	if (!c) return SPHIP_E_INVALID;
	static const size_t in_b[14] = { 4, 4, 20, 40, 60, 12, 48, 96, 32, 12, 32, 72, 84, 120 }, out_b[14] = { 8, 4, 16, 12, 4, 4, 8, 24, 24, 16, 24, 32, 24, 24 };
	if (what < 0 || what > 13 || !in || !out || n == 0 || n > 0x7fffffffull) return fail(c, SPHIP_E_INVALID, "bad selftest arguments (what=%d n=%zu)", what, n);
	sphip_ctx* k = c->kids.empty() ? c : c->kids[0];
	if ((what == 9 || what == 10) && !k->have_env) return fail(c, SPHIP_E_STATE, "selftest %d needs an environment map (sphip_set_environment)", what);
	if (what == 12 && !k->have_tex) return fail(c, SPHIP_E_STATE, "selftest %d needs an atlas (sphip_set_texture)", what);
	if (what == 13 && !k->have_nmap) return fail(c, SPHIP_E_STATE, "selftest %d needs a normal map (sphip_set_normal_map)", what);
	HIP_TRY(c, hipSetDevice(k->device));
	sp::EnvMap em{};
	if (what == 10) {                                                // T alone: the tables of the map itself, no scene needed
		em = sp::EnvMap{ (const float*)k->env_tex.p, (const double*)k->env_rc.p, (const double*)k->env_marg.p, (const float*)k->env_tpdf.p, 0.0, k->env_n };
		HIP_TRY(c, hipMemcpyAsync(&em.T, (const double*)k->env_marg.p + (k->env_n - 1u), 8, hipMemcpyDeviceToHost, k->own_stream));
		HIP_TRY(c, hipStreamSynchronize(k->own_stream));
	}
	void *d_in = nullptr, *d_out = nullptr;
	HIP_TRY(c, hipMalloc(&d_in, n * in_b[what]));
	hipError_t e = hipMalloc(&d_out, n * out_b[what]);
	if (e == hipSuccess) e = hipMemcpy(d_in, in, n * in_b[what], hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		if (what == 13) hipLaunchKernelGGL(sp::k_selftest_nmap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const float*)d_in, (uint32_t)n, (const float*)k->nmap.p, k->nmap_w, k->nmap_h, (float*)d_out);
		else if (what == 12) hipLaunchKernelGGL(sp::k_selftest_tex, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const float*)d_in, (uint32_t)n, (const float*)k->atlas.p, k->tex_w, k->tex_h, (float*)d_out);
		else if (what == 11) hipLaunchKernelGGL(sp::k_selftest_gloss, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const double*)d_in, (uint32_t)n, (float*)d_out);
		else if (what == 10) hipLaunchKernelGGL(sp::k_selftest_env_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const double*)d_in, (uint32_t)n, em, (float*)d_out);
		else if (what == 9) hipLaunchKernelGGL(sp::k_selftest_env_lookup, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const float*)d_in, (uint32_t)n, k->env_n, (float*)d_out);
		else if (what == 8) hipLaunchKernelGGL(sp::k_selftest_glass, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const float*)d_in, (uint32_t)n, (float*)d_out);
		else if (what == 7) hipLaunchKernelGGL(sp::k_selftest_shade, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, (const float*)d_in, (uint32_t)n, (float*)d_out);
		else if (what == 6) hipLaunchKernelGGL(sp::cylm256::k_selftest_cylm, dim3((unsigned)n), dim3(64), 0, k->own_stream, (const float*)d_in, (uint32_t)n, (float*)d_out);
		else hipLaunchKernelGGL(sp::k_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->own_stream, what, (const void*)d_in, (uint32_t)n, d_out);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipStreamSynchronize(k->own_stream);
	if (e == hipSuccess) e = hipMemcpy(out, d_out, n * out_b[what], hipMemcpyDeviceToHost);
	(void)hipFree(d_in);
	if (d_out) (void)hipFree(d_out);
	if (e != hipSuccess) return fail(c, SPHIP_E_DEVICE, "selftest failed: %s", hipGetErrorString(e));
	return SPHIP_OK;
}

int sphip_selftest_stage1(sphip_t* c, const float* rays, size_t n_rays, uint32_t* out_words, uint32_t* out_tri, int32_t* out_order, uint32_t* tiles_out) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->kids.empty()) return fail(c, SPHIP_E_STATE, "sphip_selftest_stage1 needs a single-device context (sphip_create)");
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "sphip_selftest_stage1 called before a scene was set");
	if (!tiles_out) return fail(c, SPHIP_E_INVALID, "tiles_out is NULL");
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	int rc = ensure_cylm(c, st);
	if (rc) return rc;
	uint32_t hdr[8];
	HIP_TRY(c, hipMemcpyAsync(hdr, c->cylm_hdr.p, sizeof hdr, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	const uint32_t tiles = hdr[6];
	const uint32_t T = c->cylm_wide ? sp::cylm512::kMTile : sp::cylm256::kMTile, W = c->cylm_wide ? sp::cylm512::kMWords : sp::cylm256::kMWords;
	const uint32_t grp8 = (c->cylm_wide ? sp::cylm512::kMGrp : sp::cylm256::kMGrp) == 8u ? 1u : 0u;
	*tiles_out = tiles | (T << 20) | (grp8 << 31);         // tiles of the stream (low 20 bits), triangles per tile, bit 31: one bit per octet (else per quad)
	if (!out_words) return SPHIP_OK;
	if (!rays || !out_order || n_rays == 0 || n_rays % 64 || n_rays > 0x7fffffffull) return fail(c, SPHIP_E_INVALID, "bad stage-1 selftest arguments (n_rays=%zu)", n_rays);
	const size_t words_b = n_rays * tiles * 2 * W * sizeof(uint32_t), tri_b = n_rays * tiles * 2 * (T / 64) * sizeof(uint32_t),
	             order_b = (size_t)tiles * T * sizeof(int32_t);
	void *d_rays = nullptr, *d_words = nullptr, *d_order = nullptr, *d_tri = nullptr;
	hipError_t e = hipMalloc(&d_rays, n_rays * 24);
	if (e == hipSuccess) e = hipMalloc(&d_words, words_b);
	if (e == hipSuccess && out_tri) e = hipMalloc(&d_tri, tri_b);
	if (e == hipSuccess) e = hipMalloc(&d_order, order_b);
	if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, n_rays * 24, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		sp::CylStream cs{ (const float4*)c->cylm_rec.p, (const uint32_t*)c->cylm_hdr.p, (const float4*)c->cylm_big.p };
		hipLaunchKernelGGL(c->cylm_wide ? sp::cylm512::k_selftest_stage1 : sp::cylm256::k_selftest_stage1, dim3((unsigned)(n_rays / 64)), dim3(64), 0, st,
		                   (const float*)d_rays, (uint32_t)n_rays, cs, (const unsigned int*)c->bounds.p, (const float*)c->tris.p, (uint32_t)c->n_tris,
		                   (uint32_t*)d_words, (uint32_t*)d_tri, (int*)d_order);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out_words, d_words, words_b, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(out_order, d_order, order_b, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && out_tri) e = hipMemcpyAsync(out_tri, d_tri, tri_b, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (d_rays) (void)hipFree(d_rays);
	if (d_words) (void)hipFree(d_words);
	if (d_order) (void)hipFree(d_order);
	if (d_tri) (void)hipFree(d_tri);
	if (e != hipSuccess) return fail(c, SPHIP_E_DEVICE, "stage-1 selftest failed: %s", hipGetErrorString(e));
	return SPHIP_OK;
}

int sphip_selftest_retest(sphip_t* c, const float* rays, size_t n_rays, uint8_t* out_bits, int32_t* out_order, uint32_t* tiles_out) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->kids.empty()) return fail(c, SPHIP_E_STATE, "sphip_selftest_retest needs a single-device context (sphip_create)");
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "sphip_selftest_retest called before a scene was set");
	if (!tiles_out) return fail(c, SPHIP_E_INVALID, "tiles_out is NULL");
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	int rc = ensure_cylm(c, st);
	if (rc) return rc;
	uint32_t hdr[8];
	HIP_TRY(c, hipMemcpyAsync(hdr, c->cylm_hdr.p, sizeof hdr, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	const uint32_t tiles = hdr[6];
	const uint32_t T = c->cylm_wide ? sp::cylm512::kMTile : sp::cylm256::kMTile;
	const uint32_t grp8 = (c->cylm_wide ? sp::cylm512::kMGrp : sp::cylm256::kMGrp) == 8u ? 1u : 0u;
	*tiles_out = tiles | (T << 20) | (grp8 << 31);         // as sphip_selftest_stage1
	if (!out_bits) return SPHIP_OK;
	if (!rays || !out_order || n_rays == 0 || n_rays % 64 || n_rays > 0x7fffffffull) return fail(c, SPHIP_E_INVALID, "bad re-test selftest arguments (n_rays=%zu)", n_rays);
	const size_t bits_b = n_rays * tiles * (T / 4), order_b = (size_t)tiles * T * sizeof(int32_t);
	void *d_rays = nullptr, *d_bits = nullptr, *d_order = nullptr;
	hipError_t e = hipMalloc(&d_rays, n_rays * 24);
	if (e == hipSuccess) e = hipMalloc(&d_bits, bits_b ? bits_b : 1);
	if (e == hipSuccess) e = hipMalloc(&d_order, order_b ? order_b : 1);
	if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, n_rays * 24, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		sp::CylStream cs{ (const float4*)c->cylm_rec.p, (const uint32_t*)c->cylm_hdr.p, (const float4*)c->cylm_big.p };
		hipLaunchKernelGGL(c->cylm_wide ? sp::cylm512::k_selftest_retest : sp::cylm256::k_selftest_retest, dim3((unsigned)(n_rays / 64)), dim3(64), 0, st,
		                   (const float*)d_rays, (uint32_t)n_rays, cs, (const unsigned int*)c->bounds.p, (unsigned char*)d_bits, (int*)d_order);
		e = hipGetLastError();
	}
	if (e == hipSuccess && bits_b) e = hipMemcpyAsync(out_bits, d_bits, bits_b, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && order_b) e = hipMemcpyAsync(out_order, d_order, order_b, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (d_rays) (void)hipFree(d_rays);
	if (d_bits) (void)hipFree(d_bits);
	if (d_order) (void)hipFree(d_order);
	if (e != hipSuccess) return fail(c, SPHIP_E_DEVICE, "re-test selftest failed: %s", hipGetErrorString(e));
	return SPHIP_OK;
}

// The sort uses c->sort_kv and c->sort_hist as the builders do.  Both are scratch of a build: build_cylm and ensure_bvh read the sorted
// half while they lay out cylm_rec / bvh_rec / bvh_idx / bvh_nodes and keep no pointer into either buffer afterwards (CylStream and BvhArgs
// name only the laid-out buffers), so a sort between two renders leaves every built stream valid.
int sphip_selftest_sort(sphip_t* c, const uint32_t* keys, const uint32_t* vals, size_t n, uint32_t key_bits, uint32_t* out_keys, uint32_t* out_vals) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->kids.empty()) return fail(c, SPHIP_E_STATE, "sphip_selftest_sort needs a single-device context (sphip_create)");
	if (!keys || !vals || !out_keys || !out_vals || n == 0 || n > 0x0fffffffull || key_bits == 0 || key_bits > 32)
		return fail(c, SPHIP_E_INVALID, "bad sort selftest arguments (n=%zu key_bits=%u)", n, key_bits);
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	int rc = ensure(c, c->sort_kv, n * 16);
	if (rc) return rc;
	uint32_t* kv = (uint32_t*)c->sort_kv.p;
	HIP_TRY(c, hipMemcpyAsync(kv, keys, n * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipMemcpyAsync(kv + 2 * n, vals, n * 4, hipMemcpyHostToDevice, st));
	int half = 0;
	if ((rc = radix_sort(c, (uint32_t)n, key_bits, st, &half))) return rc;
	HIP_TRY(c, hipMemcpyAsync(out_keys, kv + (size_t)half * n, n * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(out_vals, kv + (size_t)(2 + half) * n, n * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	return SPHIP_OK;
}

int sphip_selftest_bvh_dump(sphip_t* c, uint32_t* n_leaves_out, uint32_t* out_meta, float* out_nodes, float* out_rec, int32_t* out_idx) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->kids.empty()) return fail(c, SPHIP_E_STATE, "sphip_selftest_bvh_dump needs a single-device context (sphip_create)");
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "sphip_selftest_bvh_dump called before a scene was set");
	if (!n_leaves_out) return fail(c, SPHIP_E_INVALID, "n_leaves_out is NULL");
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	int rc = ensure_bvh(c, st);
	if (rc) return rc;
	const size_t nl = c->bvh_leaves, slots = nl * 4 + sp::kBvhMaxBig;
	*n_leaves_out = c->bvh_leaves;
	if (out_meta) HIP_TRY(c, hipMemcpyAsync(out_meta, c->bvh_meta.p, 16 * 4, hipMemcpyDeviceToHost, st));
	if (out_nodes) HIP_TRY(c, hipMemcpyAsync(out_nodes, c->bvh_nodes.p, 2 * nl * 32, hipMemcpyDeviceToHost, st));
	if (out_rec) HIP_TRY(c, hipMemcpyAsync(out_rec, c->bvh_rec.p, slots * 48, hipMemcpyDeviceToHost, st));
	if (out_idx) HIP_TRY(c, hipMemcpyAsync(out_idx, c->bvh_idx.p, slots * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	return SPHIP_OK;
}

int sphip_selftest_env_dump(sphip_t* c, uint32_t* n_out, double* out_wt, double* out_rc, double* out_marg, float* out_tpdf, double* out_T_wenv_W) {
	if (!c) return SPHIP_E_INVALID;
	if (!n_out) return fail(c, SPHIP_E_INVALID, "n_out is NULL");
	sphip_ctx* k = c->kids.empty() ? c : c->kids[0];
	if (!k->have_scene) return fail(c, SPHIP_E_STATE, "sphip_selftest_env_dump called before a scene was set");
	if (!k->have_env) return fail(c, SPHIP_E_STATE, "sphip_selftest_env_dump needs an environment map (sphip_set_environment)");
	HIP_TRY(c, hipSetDevice(k->device));
	hipStream_t st = k->own_stream;
	if (const int rc = ensure_env_lights(k, st)) return k == c ? rc : fail(c, rc, "device %d: %s", k->device, k->err.c_str());
	const size_t n = k->env_n, nn = n * n;
	*n_out = k->env_n;
	if (out_wt) HIP_TRY(c, hipMemcpyAsync(out_wt, k->env_wt.p, nn * 8, hipMemcpyDeviceToHost, st));
	if (out_rc) HIP_TRY(c, hipMemcpyAsync(out_rc, k->env_rc.p, nn * 8, hipMemcpyDeviceToHost, st));
	if (out_marg) HIP_TRY(c, hipMemcpyAsync(out_marg, k->env_marg.p, n * 8, hipMemcpyDeviceToHost, st));
	if (out_tpdf) HIP_TRY(c, hipMemcpyAsync(out_tpdf, k->env_tpdf.p, nn * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	if (out_T_wenv_W) { out_T_wenv_W[0] = k->env_T; out_T_wenv_W[1] = k->env_wenv; out_T_wenv_W[2] = k->env_W; }
	return SPHIP_OK;
}

int sphip_selftest_bvh_walk(sphip_t* c, const float* rays, size_t n_rays, const int32_t* src_idx, const float* tmax, int any_hit,
                            int32_t* out_idx, float* out_d, uint32_t* out_steps, uint32_t* out_leaves) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->kids.empty()) return fail(c, SPHIP_E_STATE, "sphip_selftest_bvh_walk needs a single-device context (sphip_create)");
	if (!c->have_scene) return fail(c, SPHIP_E_STATE, "sphip_selftest_bvh_walk called before a scene was set");
	if (!rays || !out_idx || !out_d || !out_steps || !out_leaves || n_rays == 0 || n_rays > 0x7fffffffull)
		return fail(c, SPHIP_E_INVALID, "bad BVH walk selftest arguments (n_rays=%zu)", n_rays);
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	int rc = ensure_bvh(c, st);
	if (rc) return rc;
	// one allocation: rays | src | tmax | idx | d | steps | leaves
	const size_t n = n_rays;
	char* d_all = nullptr;
	HIP_TRY(c, hipMalloc((void**)&d_all, n * (24 + 6 * 4)));
	float* d_rays = (float*)d_all;
	int* d_src = (int*)(d_all + n * 24);
	float* d_tmax = (float*)(d_all + n * 28);
	int* d_idx = (int*)(d_all + n * 32);
	float* d_d = (float*)(d_all + n * 36);
	uint32_t *d_steps = (uint32_t*)(d_all + n * 40), *d_leaves = (uint32_t*)(d_all + n * 44);
	hipError_t e = hipMemcpyAsync(d_rays, rays, n * 24, hipMemcpyHostToDevice, st);
	if (e == hipSuccess && src_idx) e = hipMemcpyAsync(d_src, src_idx, n * 4, hipMemcpyHostToDevice, st);
	if (e == hipSuccess && tmax) e = hipMemcpyAsync(d_tmax, tmax, n * 4, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		sp::BvhArgs B{};
		B.nodes = (const float4*)c->bvh_nodes.p; B.leaf_rec = (const float4*)c->bvh_rec.p; B.leaf_idx = (const int*)c->bvh_idx.p;
		B.n_leaves = c->bvh_leaves; B.first_leaf = c->bvh_leaves; B.meta = (const uint32_t*)c->bvh_meta.p;
		hipLaunchKernelGGL(sp::k_selftest_bvh_walk, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)d_rays, (uint32_t)n, B,
		                   src_idx ? (const int*)d_src : nullptr, tmax ? (const float*)d_tmax : nullptr, any_hit, d_idx, d_d, d_steps, d_leaves);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out_idx, d_idx, n * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(out_d, d_d, n * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(out_steps, d_steps, n * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(out_leaves, d_leaves, n * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	(void)hipFree(d_all);
	if (e != hipSuccess) return fail(c, SPHIP_E_DEVICE, "BVH walk selftest failed: %s", hipGetErrorString(e));
	return SPHIP_OK;
}

void sphip_denoise_defaults(sphip_denoise* out) {
	if (!out) return;
	std::memset(out, 0, sizeof *out);
	out->iterations = 5;           // calibrated with tools/denoise_time.py
	out->normal_log2 = 7;
	out->sigma_depth = 0.1f;
	out->sigma_lum = 4.0f;
}

int sphip_gbuffer_device(sphip_t* c, const void* d_rays, size_t n_rays, int flags, void* d_out_gbuf, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	HIP_TRY(c, hipSetDevice(c->device));
	c->timed_upload = c->timed_download = false;
	return gbuffer_dev(c, d_rays, n_rays, flags, d_out_gbuf, (hipStream_t)stream);
}

int sphip_denoise_device(sphip_t* c, const sphip_denoise* P, size_t w, size_t h, const void* d_mean, const void* d_var, const void* d_gbuf,
                         void* d_out_rgba, void* d_out_rgb, void* stream) {
	if (!c) return SPHIP_E_INVALID;
	int rc;
	if ((rc = check_denoise(c, P))) return rc;
	if ((rc = single_device_entry(c))) return rc;
	if (!d_mean || !d_gbuf || !d_out_rgba) return fail(c, SPHIP_E_INVALID, "null mean, G-buffer or output pointer");
	if (w == 0 || h == 0 || w >= (1u << 30) || h >= (1u << 30) || w * h > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "bad image size (w=%zu h=%zu)", w, h);
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = (hipStream_t)stream;
	const size_t n = w * h;
	if ((rc = ensure(c, c->dn_a, n * 16)) || (rc = ensure(c, c->dn_b, n * 16)) || (rc = dn_clock_start(c, st))) return rc;
	const bool k0 = P->iterations == 0;
	hipLaunchKernelGGL(sp::k_dn_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)d_mean, (const float*)d_var, (uint32_t)n,
	                   k0 ? (float4*)nullptr : (float4*)c->dn_a.p, k0 ? (uint32_t*)d_out_rgba : nullptr, k0 ? (float*)d_out_rgb : nullptr);
	HIP_TRY(c, hipGetLastError());
	c->stats.n_launches = 1;
	if ((rc = atrous_run(c, c->dn_a, c->dn_b, P, w, h, d_var != nullptr, d_gbuf, (uint32_t*)d_out_rgba, (float*)d_out_rgb, st, &c->stats.n_launches))) return rc;
	HIP_TRY(c, hipEventRecord(c->ev_k1, st));
	c->timed_upload = c->timed_download = false;
	note_render(c, st, n, (int)c->stats.kernel_variant);       // the variant of the last render stays
	return SPHIP_OK;
}

int sphip_accum_gbuffer(sphip_t* c, void* out_gbuf) {
	if (!c) return SPHIP_E_INVALID;
	if (!out_gbuf) return fail(c, SPHIP_E_INVALID, "null G-buffer output");
	if (!c->acc_on) return fail(c, SPHIP_E_STATE, "sphip_accum_gbuffer called with no accumulation begun");
	if (c->acc_stale) return fail(c, SPHIP_E_STATE, "the scene changed since sphip_accum_begin: begin a new accumulation");
	const size_t n = c->acc_w * c->acc_h;
	if (!c->kids.empty()) {
		// the whole frame's rays on the first device, as the denoiser builds it there
		const int g = (int)c->kids.size();
		const RowPlan plan(c->acc_w, c->acc_h, g, (size_t)plan_tile_rows(c->acc_h, g));
		std::vector<float> rays(n * 6);
		int rc;
		if ((rc = read_shards(c, plan, { { &sphip_ctx::acc_rays, 24, rays.data() } }))) return rc;
		sphip_ctx* root = c->kids[0];
		HIP_TRY(c, hipSetDevice(root->device));
		if ((rc = ensure(c, c->dn_rays, n * 24)) || (rc = ensure(c, c->dn_gbuf, n * 32))) return rc;
		HIP_TRY(c, hipMemcpyAsync(c->dn_rays.p, rays.data(), n * 24, hipMemcpyHostToDevice, root->own_stream));
		if (!c->dn_gbuf_ok && (rc = gbuffer_dev(root, c->dn_rays.p, n, c->acc_flags, c->dn_gbuf.p, root->own_stream))) {
			(void)hipStreamSynchronize(root->own_stream);
			return fail(c, rc, "device %d: %s", root->device, root->err.c_str());
		}
		c->dn_gbuf_ok = true;
		HIP_TRY(c, hipMemcpyAsync(out_gbuf, c->dn_gbuf.p, n * 32, hipMemcpyDeviceToHost, root->own_stream));
		HIP_TRY(c, hipStreamSynchronize(root->own_stream));
		return SPHIP_OK;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	int rc;
	if ((rc = ensure(c, c->dn_gbuf, n * 32))) return rc;
	if (!c->dn_gbuf_ok && (rc = gbuffer_dev(c, c->acc_rays.p, n, c->acc_flags, c->dn_gbuf.p, st))) { (void)hipStreamSynchronize(st); return rc; }
	c->dn_gbuf_ok = true;
	HIP_TRY(c, hipMemcpyAsync(out_gbuf, c->dn_gbuf.p, n * 32, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	return SPHIP_OK;
}

int sphip_accum_denoise(sphip_t* c, const sphip_denoise* P, uint8_t* out_rgba, float* out_rgb) {
	if (!c) return SPHIP_E_INVALID;
	int rc;
	if ((rc = check_denoise(c, P))) return rc;
	if (!out_rgba) return fail(c, SPHIP_E_INVALID, "null output pointer");
	if (!c->acc_on || c->acc_total == 0) return fail(c, SPHIP_E_STATE, "sphip_accum_denoise needs an accumulation with at least one step");
	if (c->acc_stale) return fail(c, SPHIP_E_STATE, "the scene changed since sphip_accum_begin: begin a new accumulation");
	if (c->acc_w >= (1u << 30) || c->acc_h >= (1u << 30)) return fail(c, SPHIP_E_INVALID, "image too wide or tall for the filter");
	if (!c->kids.empty()) return multi_accum_denoise(c, P, out_rgba, out_rgb);
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	const size_t n = c->acc_w * c->acc_h;
	rc = accum_denoise_dev(c, c, P, c->acc_rays.p, false, c->adp_on, out_rgb != nullptr, st);
	if (!rc) {
		if (hipMemcpyAsync(out_rgba, c->rgba.p, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    (out_rgb && hipMemcpyAsync(out_rgb, c->accum.p, n * 12, hipMemcpyDeviceToHost, st) != hipSuccess) ||
		    hipStreamSynchronize(st) != hipSuccess) rc = fail(c, SPHIP_E_DEVICE, "denoise readback failed: %s", hipGetErrorString(hipGetLastError()));
	}
	if (rc) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); return rc; }
	c->timed_upload = c->timed_download = false;
	return SPHIP_OK;
}

void sphip_reproject_defaults(sphip_reproject* out) {
	if (!out) return;
	std::memset(out, 0, sizeof *out);
	out->max_history = 32.0f;      // calibrated with tools/reproject_calibrate.py
	out->normal_min = 0.5f;
	out->plane_tol = 0.1f;
}

int sphip_reproject_device(sphip_t* c, const sphip_reproject* P, const sphip_camera* cam_prev, size_t w, size_t h, const void* d_rays_cur,
                           const void* d_gbuf_cur, const void* d_rays_prev, const void* d_gbuf_prev, const void* d_mean_prev, const void* d_hist_prev,
                           void* d_out_mean, void* d_out_hist, void* stream) {
	if (!c) return SPHIP_E_INVALID;
	int rc;
	if ((rc = check_reproject(c, P))) return rc;
	if ((rc = single_device_entry(c))) return rc;
	if (!cam_prev || !d_rays_cur || !d_gbuf_cur || !d_rays_prev || !d_gbuf_prev || !d_mean_prev || !d_hist_prev || !d_out_mean || !d_out_hist)
		return fail(c, SPHIP_E_INVALID, "null camera, input or output pointer");
	if (w == 0 || h == 0 || w >= (1u << 30) || h >= (1u << 30) || w * h > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "bad image size (w=%zu h=%zu)", w, h);
	if (cam_prev->res_x != w || cam_prev->res_y != h)
		return fail(c, SPHIP_E_INVALID, "w x h = %zux%zu differs from the previous camera's %ux%u", w, h, cam_prev->res_x, cam_prev->res_y);
	if (((uintptr_t)d_gbuf_cur | (uintptr_t)d_gbuf_prev) & 15u) return fail(c, SPHIP_E_INVALID, "a G-buffer pointer is not 16-byte aligned");
	HIP_TRY(c, hipSetDevice(c->device));
	return reproject_dev(c, P, cam_prev, w, h, d_rays_cur, d_gbuf_cur, d_rays_prev, d_gbuf_prev, d_mean_prev, d_hist_prev, d_out_mean, d_out_hist,
	                     (hipStream_t)stream);
}

int sphip_temporal_resolve_device(sphip_t* c, size_t n, const void* d_sum, uint32_t n_samples, const void* d_hist_mean, const void* d_hist,
                                  void* d_out_rgba, void* d_out_mean, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	if (!d_sum || (!d_out_rgba && !d_out_mean)) return fail(c, SPHIP_E_INVALID, "null sum pointer, or no output");
	if ((d_hist_mean == nullptr) != (d_hist == nullptr)) return fail(c, SPHIP_E_INVALID, "a history is both its mean and its count, or neither");
	if (n == 0 || n > 0xffffffffull || n_samples == 0) return fail(c, SPHIP_E_INVALID, "n = %zu pixels of %u samples: both must be positive", n, n_samples);
	HIP_TRY(c, hipSetDevice(c->device));
	return temporal_resolve_dev(c, n, d_sum, n_samples, d_hist_mean, d_hist, d_out_rgba, d_out_mean, (hipStream_t)stream, false);
}

int sphip_accum_reproject(sphip_t* c, const sphip_camera* cam_new, uint64_t seed, const sphip_reproject* P) {
	if (!c) return SPHIP_E_INVALID;
	int rc;
	if (!cam_new) return fail(c, SPHIP_E_INVALID, "null camera");
	if ((rc = check_reproject(c, P))) return rc;
	if (!c->kids.empty()) return fail(c, SPHIP_E_STATE, "sphip_accum_reproject needs a single-device context (sphip_create)");
	if (!c->acc_on) return fail(c, SPHIP_E_STATE, "sphip_accum_reproject called with no accumulation begun");
	if (c->acc_stale) return fail(c, SPHIP_E_STATE, "the scene changed since sphip_accum_begin: begin a new accumulation");
	if (!c->acc_has_cam) return fail(c, SPHIP_E_STATE, "sphip_accum_reproject needs an accumulation begun with a camera, not with rays");
	if (c->adp_on) return fail(c, SPHIP_E_STATE, "sphip_accum_reproject needs a plain accumulation, not an adaptive one");
	if (c->acc_total == 0) return fail(c, SPHIP_E_STATE, "sphip_accum_reproject needs an accumulation with at least one step");
	if (cam_new->res_x != c->acc_w || cam_new->res_y != c->acc_h)
		return fail(c, SPHIP_E_INVALID, "the camera's %ux%u differs from the accumulation's %zux%zu", cam_new->res_x, cam_new->res_y, c->acc_w, c->acc_h);
	if (c->acc_w >= (1u << 30) || c->acc_h >= (1u << 30)) return fail(c, SPHIP_E_INVALID, "image too wide or tall to reproject");
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	const size_t w = c->acc_w, h = c->acc_h, n = w * h;
	auto body = [&]() -> int {
		int r;
		if ((r = ensure(c, c->rp_hmean, n * 12)) || (r = ensure(c, c->rp_hist, n * 4)) || (r = ensure(c, c->rp_prays, n * 24)) ||
		    (r = ensure(c, c->rp_pgbuf, n * 32)) || (r = ensure(c, c->rp_pmean, n * 12)) || (r = ensure(c, c->rp_phist, n * 4)) ||
		    (r = ensure(c, c->dn_gbuf, n * 32))) return r;
		// the view being left: its G-buffer (cached, or built now), its rays, and the accumulation as a (mean, count) pair
		if (!c->dn_gbuf_ok && (r = gbuffer_dev(c, c->acc_rays.p, n, c->acc_flags, c->dn_gbuf.p, st))) return r;
		HIP_TRY(c, hipMemcpyAsync(c->rp_pgbuf.p, c->dn_gbuf.p, n * 32, hipMemcpyDeviceToDevice, st));
		HIP_TRY(c, hipMemcpyAsync(c->rp_prays.p, c->acc_rays.p, n * 24, hipMemcpyDeviceToDevice, st));
		hipLaunchKernelGGL(sp::k_history, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)c->acc_sum.p,
		                   (float)(1.0 / (double)c->acc_total), (float)c->acc_total, c->acc_hist_on ? (const float*)c->rp_hmean.p : nullptr,
		                   c->acc_hist_on ? (const float*)c->rp_hist.p : nullptr, (uint32_t)n, (float*)c->rp_pmean.p, (float*)c->rp_phist.p);
		HIP_TRY(c, hipGetLastError());
		// the new view: rays over the old ones, G-buffer over the old one, then the history the steps to come blend with
		c->dn_gbuf_ok = false;
		if ((r = launch_viewport(c, cam_new, c->acc_rays.p, st)) || (r = gbuffer_dev(c, c->acc_rays.p, n, c->acc_flags, c->dn_gbuf.p, st))) return r;
		c->dn_gbuf_ok = true;
		if ((r = reproject_dev(c, P, &c->acc_cam, w, h, c->acc_rays.p, c->dn_gbuf.p, c->rp_prays.p, c->rp_pgbuf.p, c->rp_pmean.p, c->rp_phist.p,
		                       c->rp_hmean.p, c->rp_hist.p, st))) return r;
		HIP_TRY(c, hipStreamSynchronize(st));
		return SPHIP_OK;
	};
	if ((rc = body())) {                           // the old view's state is partly overwritten: nothing can continue from it
		(void)hipStreamSynchronize(st); (void)hipGetLastError();
		c->acc_on = false;
		return rc;
	}
	c->acc_cam = *cam_new;
	c->acc_seed = seed;
	c->acc_total = 0;                              // the next step's sample_base: the sum buffer's contents are not read
	c->acc_hist_on = true;
	c->timed_upload = c->timed_download = false;
	return SPHIP_OK;
}

int sphip_accum_history(sphip_t* c, float* out_hist) {
	if (!c) return SPHIP_E_INVALID;
	if (!c->acc_on) return fail(c, SPHIP_E_STATE, "sphip_accum_history called with no accumulation begun");
	if (!out_hist) return fail(c, SPHIP_E_INVALID, "null history output");
	const size_t n = c->acc_w * c->acc_h;
	if (!c->acc_hist_on) {
		std::fill(out_hist, out_hist + n, 0.0f);
		return SPHIP_OK;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipMemcpyAsync(out_hist, c->rp_hist.p, n * 4, hipMemcpyDeviceToHost, c->own_stream));
	HIP_TRY(c, hipStreamSynchronize(c->own_stream));
	return SPHIP_OK;
}

void sphip_display_defaults(sphip_display* out) {
	if (!out) return;
	std::memset(out, 0, sizeof *out);
	out->exposure = 1.0f;          // conventions, not measurements
	out->white = 4.0f;
	out->curve = SPHIP_CURVE_FILMIC;
	out->encode = SPHIP_ENCODE_SRGB;
}

void sphip_metering_defaults(sphip_metering* out) {
	if (!out) return;
	std::memset(out, 0, sizeof *out);
	out->key = 0.18f;              // conventions as well: middle grey, the median to the 95th percentile
	out->low = 0.5f;
	out->high = 0.95f;
}

void sphip_srgb_thresholds(float out[255]) {
	if (out) std::memcpy(out, kSrgbBits, sizeof kSrgbBits);
}

int sphip_exposure_from_histogram(const uint32_t* hist, const sphip_metering* m, float* exposure_out) {
	if (!hist || !exposure_out) return fail(nullptr, SPHIP_E_INVALID, "null histogram or output pointer");
	if (const int rc = check_metering(nullptr, m)) return rc;
	*exposure_out = exposure_from_histogram(hist, m);
	return SPHIP_OK;
}

int sphip_luminance_histogram_device(sphip_t* c, size_t n, const void* d_mean, void* d_out_hist, void* stream) {
	if (const int rc = single_device_entry(c)) return rc;
	if (!d_mean || !d_out_hist) return fail(c, SPHIP_E_INVALID, "null mean or histogram pointer");
	if (n == 0 || n > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "n = %zu pixels out of range", n);
	HIP_TRY(c, hipSetDevice(c->device));
	return histogram_dev(c, n, d_mean, d_out_hist, (hipStream_t)stream);
}

int sphip_display_device(sphip_t* c, const sphip_display* p, size_t n, const void* d_mean, void* d_out_rgba, void* d_out_rgb, void* stream) {
	if (!c) return SPHIP_E_INVALID;
	int rc;
	if ((rc = check_display(c, p))) return rc;
	if ((rc = single_device_entry(c))) return rc;
	if (!d_mean || !d_out_rgba) return fail(c, SPHIP_E_INVALID, "null mean or output pointer");
	if (n == 0 || n > 0xffffffffull) return fail(c, SPHIP_E_INVALID, "n = %zu pixels out of range", n);
	HIP_TRY(c, hipSetDevice(c->device));
	return display_dev(c, p, p->exposure, n, d_mean, d_out_rgba, d_out_rgb, (hipStream_t)stream);
}

int sphip_accum_display(sphip_t* c, const sphip_display* p, const sphip_metering* m, const sphip_denoise* dn, uint8_t* out_rgba, float* out_rgb,
                        float* exposure_out) {
	if (!c) return SPHIP_E_INVALID;
	int rc;
	if ((rc = check_display(c, p)) || (m && (rc = check_metering(c, m))) || (dn && (rc = check_denoise(c, dn)))) return rc;
	if (!out_rgba) return fail(c, SPHIP_E_INVALID, "null output pointer");
	if (!c->acc_on || c->acc_total == 0) return fail(c, SPHIP_E_STATE, "sphip_accum_display needs an accumulation with at least one step");
	if (c->acc_stale) return fail(c, SPHIP_E_STATE, "the scene changed since sphip_accum_begin: begin a new accumulation");
	if (c->acc_w >= (1u << 30) || c->acc_h >= (1u << 30)) return fail(c, SPHIP_E_INVALID, "image too wide or tall for the filter");
	float E = p->exposure;
	if (!c->kids.empty()) {
		const DisplayTail post{ p, m, &E };
		if ((rc = multi_accum_denoise(c, dn, out_rgba, out_rgb, &post))) return rc;
		if (exposure_out) *exposure_out = E;
		return SPHIP_OK;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	hipStream_t st = c->own_stream;
	const size_t n = c->acc_w * c->acc_h;
	// the mean sphip_accum_step returns (plain, adaptive or blended with a history), or sphip_accum_denoise's output, in c->accum
	if (!(rc = accum_denoise_dev(c, c, dn, c->acc_rays.p, false, c->adp_on, true, st)) &&
	    !(rc = display_tail(c, p, m, n, out_rgb != nullptr, st, &E))) {
		if (hipMemcpyAsync(out_rgba, c->rgba.p, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    (out_rgb && hipMemcpyAsync(out_rgb, c->dp_rgb.p, n * 12, hipMemcpyDeviceToHost, st) != hipSuccess) ||
		    hipStreamSynchronize(st) != hipSuccess) rc = fail(c, SPHIP_E_DEVICE, "display readback failed: %s", hipGetErrorString(hipGetLastError()));
	}
	if (rc) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); return rc; }
	c->timed_upload = c->timed_download = false;
	if (exposure_out) *exposure_out = E;
	return SPHIP_OK;
}

int sphip_get_stats(sphip_t* c, sphip_stats* out) {
	if (!c || !out) return SPHIP_E_INVALID;
	if (!c->kids.empty()) return multi_get_stats(c, out);
	if (!c->have_render) return fail(c, SPHIP_E_STATE, "no render has been issued yet");
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipEventSynchronize(c->ev_k1));
	float ms = 0.0f;
	HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_k0, c->ev_k1));
	c->stats.kernel_ms = ms;
	c->stats.upload_ms = c->stats.download_ms = 0.0;
	if (c->timed_upload) { HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_u0, c->ev_u1)); c->stats.upload_ms = ms; }
	if (c->timed_download) { HIP_TRY(c, hipEventSynchronize(c->ev_d1)); HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_d0, c->ev_d1)); c->stats.download_ms = ms; }
	unsigned long long scans = 0;
	HIP_TRY(c, hipMemcpyAsync(&scans, c->counter.p, sizeof scans, hipMemcpyDeviceToHost, c->last_stream));
	HIP_TRY(c, hipStreamSynchronize(c->last_stream));
	c->stats.scans_executed = scans;
#ifdef SP_BVH_STATS
	{
		unsigned long long x[3] = {0, 0, 0};
		(void)hipMemcpy(x, c->counter.p, sizeof x, hipMemcpyDeviceToHost);
		fprintf(stderr, "[bvh stats] scans=%llu steps/scan=%.1f leaves/scan=%.1f\n", x[0], (double)x[1] / (double)(x[0] ? x[0] : 1), (double)x[2] / (double)(x[0] ? x[0] : 1));
	}
#endif
#ifdef SP_PHASE_TIMERS
	{
		unsigned long long x[16] = {};
		(void)hipMemcpy(x, c->counter.p, sizeof x, hipMemcpyDeviceToHost);
		const double tot = (double)(x[8] + x[9] + x[10] + x[11] + x[12]);
		fprintf(stderr, "[phase timers] wave-scans %llu; wave lifetime inside the scan by phase: stage 1 %.1f %%, list building + DMA issue %.1f %%, re-test rounds %.1f %%, exact turns %.1f %%, tile barrier %.1f %% (%.0f cycles per wave-scan)\n",
		        x[13], 100.0 * x[8] / tot, 100.0 * x[9] / tot, 100.0 * x[10] / tot, 100.0 * x[11] / tot, 100.0 * x[12] / tot, tot / (double)(x[13] ? x[13] : 1));
	}
#endif
#ifdef SP_FILTER_STATS
	{
		unsigned long long x[6] = {0, 0, 0, 0, 0, 0};
		(void)hipMemcpy(x, c->counter.p, sizeof x, hipMemcpyDeviceToHost);
		if (c->stats.kernel_variant >= 15)
			fprintf(stderr, "[cyl stats] group bits set=%llu stage-2 rounds(per wave)=%llu wave-tiles=%llu exact tests=%llu -> bits/lane/tile=%.3f rounds/tile=%.2f exact per bit=%.3f (= exact-test candidates per list entry: what the re-test lets through) lane utilisation in stage 2=%.3f wave-wide exact turns=%llu (%.2f per round, %.3f of their lanes used)\n",
			        x[1], x[2], x[3], x[4], (double)x[1] / (64.0 * (double)x[3]), (double)x[2] / (double)x[3], (double)x[4] / (double)x[1], (double)x[4] / (64.0 * (double)x[2]),
			        x[5], (double)x[5] / (double)x[2], (double)x[4] / (64.0 * (double)x[5]));
	}
#endif
	c->stats.n_devices = 1; c->stats.gather_kind = SPHIP_GATHER_NONE; c->stats.gather_ms = 0.0; c->stats.kernel_ms_min = c->stats.kernel_ms;
	*out = c->stats;
	return SPHIP_OK;
}

} // extern "C"
