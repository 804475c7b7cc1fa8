/* spath_hip.h -- C ABI of the MI355X (gfx950) path-tracing backend for Emanem/spath.
 *
 * This is the drop-in boundary: plain C types, caller-allocated outputs, no exceptions, no C++
 * or torch types.  It is what a `hip_renderer` peer of the reference's cpu_renderer binds to
 * (see spath_amd/host/hip_renderer.cpp and INTEGRATION.md).  Each entry point names the reference
 * interface it stands behind (paths relative to the reference repository root).
 *
 * Data layouts are the reference's tightly packed float structs:
 *   ray       6 x f32  pos.xyz dir.xyz                  geom::ray        src/geom.h:179-182
 *   triangle 12 x f32  v0 v1 v2 n                       geom::triangle   src/geom.h:185-190
 *   material  6 x f32  reflectance.rgb emittance.rgb    scene::material  src/scene.h:47-50
 *   pixel     4 x u8   r g b a(=0)                      scene::RGBA      src/scene.h:25-30
 * Pixel index = i + j*W, row 0 = top (src/view.h:112).
 *
 * Every function returning int returns 0 on success and a negative SPHIP_E_* code otherwise;
 * sphip_last_error() then describes the failure.  The C++ adapter turns a non-zero status into
 * std::runtime_error, which is how the reference's GPU peers report failure
 * (src/cl_renderer.cpp:155-187, src/vk_renderer.cpp:318-349).
 */
#ifndef SPATH_HIP_H
#define SPATH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPHIP_ABI_VERSION 3

typedef struct sphip_ctx sphip_t;

enum {
	SPHIP_OK = 0,
	SPHIP_E_INVALID = -1,   /* bad argument (NULL pointer, n_samples == 0, ...) */
	SPHIP_E_DEVICE = -2,    /* HIP runtime error (no device, allocation failure, launch failure) */
	SPHIP_E_STATE = -3      /* call order error (render before set_scene) */
};

/* render modes: which renderer virtual is being served */
enum {
	SPHIP_MODE_FLAT = 0,    /* renderer::render_flat  src/renderer.h:31, body src/cpu_renderer.cpp:81-101 */
	SPHIP_MODE_PT = 1       /* renderer::render       src/renderer.h:32, body src/cpu_renderer.cpp:29-79,118-184 */
};

/* flags (bitwise or) */
enum {
	SPHIP_KERNEL_AUTO = 0,          /* let the library pick the scan kernel */
	SPHIP_KERNEL_MASK = 0xff,       /* low byte: explicit kernel variant (see sphip_kernel_name) for A/B runs;
	                                   every variant produces bit-identical images */
	SPHIP_FLAG_PRIMARY_REUSE = 0x100,/* scan the (identical) primary ray of a pixel once for all its samples
	                                   (src/cpu_renderer.cpp:74-76 re-scans it); identical image, ~1/5 fewer scans.
	                                   With the two-stage kernels: a closest-hit pre-pass, one scan per pixel, then the
	                                   path-tracing launch (stats: one launch more).  OFF by default: the default executes
	                                   every scan the reference executes */
	SPHIP_FLAG_CHUNKS_SHIFT = 16,   /* bits 16..23: number of sample chunks of a path-traced launch, 0 = let the library
	                                   choose.  A frame (or shard) with too few pixels to fill the GPU several times over is
	                                   launched as (pixel, sample chunk) lanes; each sample's radiance goes to a scratch buffer
	                                   and a second kernel adds them up per pixel in sample order (src/cpu_renderer.cpp:74-76),
	                                   so the image is bit-identical whatever the number of chunks.  1 = never split. */
	SPHIP_FLAG_CHUNKS_MASK = 0xff0000,
	SPHIP_FLAG_ACCEL = 0x200,        /* OPT-IN acceleration structure (linear BVH).  Changes the work
	                                   definition: the reference tests every triangle (README.md:23).  Same strict triangle
	                                   test and tie rule, so every geometric hit is reproduced bit for bit; what it cannot
	                                   reproduce are the reference's rounding-noise accepts on rays almost coplanar with a
	                                   far-away triangle.  Never used by bench.py's headline figure. */
	SPHIP_FLAG_NEE = 0x400,          /* OPT-IN next-event estimation (light sampling with shadow rays) for SPHIP_MODE_PT; see
	                                   "next-event estimation" below.  Changes the estimator, not its expectation. */
	SPHIP_FLAG_MIS = 0x800,          /* OPT-IN multiple importance sampling of next-event estimation: valid only together with
	                                   SPHIP_FLAG_NEE; see "multiple importance sampling" below.  Same expectation again. */
	SPHIP_FLAG_CAMERA_SAMPLES = 0x1000, /* OPT-IN per-sample camera rays (pixel antialiasing, thin-lens depth of field) for the camera paths
	                                   of SPHIP_MODE_PT; see "camera samples" below.  Changes the image: it is no longer the reference's. */
	SPHIP_FLAG_SPECULAR = 0x2000,    /* OPT-IN mirror and mixed diffuse/mirror materials from the context's specular table
	                                   (sphip_set_specular) for SPHIP_MODE_PT; see "specular reflection" below.  Without the flag the
	                                   table is ignored. */
	SPHIP_FLAG_SMOOTH = 0x4000,      /* OPT-IN smooth shading by the context's per-vertex normals (sphip_set_vertex_normals) for
	                                   SPHIP_MODE_PT; see "smooth shading" below.  Without the flag the normals are ignored. */
	SPHIP_FLAG_DIELECTRIC = 0x8000,  /* OPT-IN transparency: dielectric (glass) triangles with Fresnel reflection and refraction from the
	                                   context's dielectric table (sphip_set_dielectric) for SPHIP_MODE_PT; see "transparency" below.
	                                   Without the flag the table is ignored. */
	SPHIP_FLAG_GLOSSY = 0x2000000,   /* OPT-IN glossy reflection: the mirror lobe of SPHIP_FLAG_SPECULAR roughened by the context's roughness
	                                   table (sphip_set_roughness) for SPHIP_MODE_PT: valid only together with SPHIP_FLAG_SPECULAR; see
	                                   "glossy reflection" below.  Without the flag the table is ignored. */
	SPHIP_FLAG_TEXTURE = 0x4000000,  /* OPT-IN textures: the diffuse reflectance of a hit scaled by the bilinear sample of the context's atlas
	                                   (sphip_set_texture) at the hit's interpolated UV (sphip_set_uv) for SPHIP_MODE_PT; see "textures"
	                                   below.  Without the flag both are ignored. */
	SPHIP_FLAG_NORMAL_MAP = 0x8000000, /* OPT-IN normal mapping: the shading normal of a hit replaced by the tangent-space normal of the
	                                   context's normal map (sphip_set_normal_map) at the hit's interpolated UV (sphip_set_uv) for
	                                   SPHIP_MODE_PT; see "normal mapping" below.  Without the flag the map is ignored. */
	SPHIP_FLAG_ENVIRONMENT = 0x1000000 /* OPT-IN environment lighting by the context's octahedral radiance map (sphip_set_environment) for
	                                   SPHIP_MODE_PT: a ray that leaves the scene carries the map's radiance, and NEE|MIS samples the map;
	                                   see "environment lighting" below.  Without the flag the map is ignored.  (Bits 16..23 are the
	                                   sample chunks.) */
};

/* Pixel-shard descriptor: which global pixel the k-th ray of a shard is.
 *   global_pixel(k) = pixel_base + (k / tile_px) * tile_stride_px + (k % tile_px)
 * A whole image is {0, npix, 0}.  Row tiles dealt round-robin to G GPUs (rank r, tile of R rows of
 * width W): {r*R*W, R*W, G*R*W}.  The global index keys the counter RNG, so an image does not
 * depend on how it was sharded. */
typedef struct {
	uint64_t pixel_base;
	uint64_t tile_px;
	uint64_t tile_stride_px;
} sphip_shard;

typedef struct {
	double   kernel_ms;        /* device time of the last render's kernels (hipEvent, on the launch stream) */
	double   upload_ms;        /* host-pointer path only: H2D of rays (+ scene when it changed) */
	double   download_ms;      /* host-pointer path only: D2H of the image */
	uint64_t scans_executed;   /* closest-hit scans (one ray against all triangles) the last render ran */
	uint64_t n_tris;
	uint64_t n_pixels;
	uint32_t kernel_variant;   /* variant that actually ran */
	uint32_t n_launches;
	/* multi-device contexts (sphip_create_multi); a single-device context reports 1, 0, 0, kernel_ms */
	uint32_t n_devices;        /* devices the last render ran on */
	uint32_t gather_kind;      /* SPHIP_GATHER_* used to bring the row tiles to the first device */
	double   gather_ms;        /* first tile copy enqueued -> image assembled on the first device (hipEvent on its stream) */
	double   kernel_ms_min;    /* kernel_ms is the slowest device's, this the fastest's */
} sphip_stats;

enum {
	SPHIP_GATHER_NONE = 0,     /* one device */
	SPHIP_GATHER_RCCL = 1,     /* ncclSend/ncclRecv group over xGMI, single-process communicator (ncclCommInitAll) */
	SPHIP_GATHER_PEER = 2      /* hipMemcpyPeerAsync per device (also what runs when a device id is listed twice, or RCCL is absent) */
};

/* ---- lifetime.  Replaces X_renderer::get(w,h) construction (src/cpu_renderer.cpp:205-209) for the
 * device-owning part; device buffers are cached grow-only in the context like
 * src/cl_renderer.cpp:107-112 and released by sphip_destroy. */
int  sphip_create(int device_id, sphip_t** out);
/* All the GPUs of one node behind ONE context, so that a renderer object registered beside cpu_renderer
 * (src/main.cpp:242-248, interface src/renderer.h:24-36) drives every device: the framebuffer is dealt to the devices as
 * interleaved pixel-row tiles (round-robin, sphip_plan_*), every device holds the whole scene and renders its tiles on its
 * own stream from its own host thread, the RGBA8 tiles are gathered to the first device (RCCL over xGMI; peer copies as the
 * fallback), un-permuted there and read back once.  The image is bit-identical to a one-device render (pixel-keyed RNG).
 *   device_ids == NULL: every visible device, or the comma-separated list in the environment variable SPATH_HIP_DEVICES.
 *   A device may be listed more than once (several shards on one GPU: how a one-GPU box exercises this path).
 *   SPATH_HIP_GATHER=rccl|peer overrides the choice of exchange.
 * The host-pointer entry points (sphip_set_scene, sphip_render, sphip_render_camera, sphip_accum_begin, sphip_accum_step,
 * sphip_accum_gbuffer, sphip_accum_denoise, sphip_accum_display, sphip_get_stats, sphip_description, sphip_destroy) accept such a context; the device-pointer entry points need a single-device context (SPHIP_E_STATE). */
int  sphip_create_multi(const int* device_ids, int n_devices, sphip_t** out);
int  sphip_device_count(const sphip_t* ctx);        /* devices behind ctx (1 for sphip_create) */
void sphip_destroy(sphip_t* ctx);
const char* sphip_last_error(const sphip_t* ctx);   /* ctx may be NULL: error of a failed sphip_create */
const char* sphip_description(const sphip_t* ctx);  /* renderer::get_description  src/renderer.h:26 */
int  sphip_abi_version(void);
const char* sphip_kernel_name(int variant);         /* NULL when the variant does not exist */
const char* sphip_build_info(void);                 /* "src=<16 hex digits>": hash of the sources and compiler flags this library was built
                                                       from (__graft_entry__.source_hash), "src=unknown" for a hand-made build; profiler-derived
                                                       figures under profiles/ carry the same stamp */
int  sphip_kernel_available(int variant);           /* 1 when the library carries the variant (1 and 2, the exact-only scans; 8, the
                                                       opt-in BVH; 15, one f32 filter scan for A/B runs; 16, the default scan), else 0:
                                                       the numbers of the retired scans keep their names and are refused */

/* ---- host-pointer path: exactly what renderer::render / render_flat receive
 * (src/renderer.h:31-32): borrowed host arrays, valid only during the call; blocking. */
int sphip_set_scene(sphip_t* ctx, const float* tris, const float* mats, size_t n_tris);
int sphip_render(sphip_t* ctx, const float* rays, size_t w, size_t h, size_t n_samples,
                 uint64_t seed, int mode, int flags,
                 uint8_t* out_rgba /* w*h*4 */, float* out_accum /* w*h*3 or NULL */);

/* ---- device-resident path: pointers are HIP device pointers on ctx's device, `stream` is a
 * hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing; outputs are complete
 * when the stream reaches the end of the enqueued work.  Used for HBM-resident benchmarking and for
 * pixel-row-tile sharding across GPUs (one context per GPU).  Stream order is the only ordering: issue
 * sphip_set_scene_device and the renders that use that scene on the same stream (or synchronise in between);
 * d_tris / d_mats are copied, so they may be freed once the stream has passed the call. */
int sphip_set_scene_device(sphip_t* ctx, const void* d_tris, const void* d_mats, size_t n_tris, void* stream);
int sphip_render_device(sphip_t* ctx, const void* d_rays /* n_rays*6 f32: the shard's rays */, size_t n_rays,
                        const sphip_shard* shard /* NULL = {0, n_rays, 0} */, size_t image_width,
                        size_t n_samples, uint64_t seed, int mode, int flags,
                        void* d_out_rgba /* n_rays*4 u8 */, void* d_out_accum /* n_rays*3 f32 or NULL */,
                        void* stream);

/* ---- device-side viewport generation (camera -> rays without the 24 B/pixel upload).
 * Same arithmetic as view::camera::get_viewport (src/view.h:94-132), float operation for float operation, so the
 * rays are bit-identical to what renderer::get_viewport hands to render().  The camera's trigonometric values are
 * computed by the caller exactly like the reference does on the host (src/view.h:77-80,87-92: std::cos/std::sin of
 * angle.y and angle.x) and passed in. */
typedef struct {
	float pos[3];                 /* view::camera::pos   (src/view.h:70) */
	float cos_y, sin_y, cos_x, sin_x;
	float focal;                  /* view::camera::focal (src/view.h:72) */
	uint32_t res_x, res_y;
} sphip_camera;

int sphip_viewport_device(sphip_t* ctx, const sphip_camera* cam, void* d_rays_out /* res_x*res_y*6 f32 */, void* stream);

/* get_viewport + render / render_flat in one call, rays never leave the device: equals
 * sphip_render(ctx, rays_of(cam), cam->res_x, cam->res_y, ...).  Blocking; host output pointers. */
int sphip_render_camera(sphip_t* ctx, const sphip_camera* cam, size_t n_samples, uint64_t seed, int mode, int flags,
                        uint8_t* out_rgba, float* out_accum);

/* The closest-hit scan on its own (the loop of src/cpu_renderer.cpp:36-49 for each ray): for ray k writes the
 * index of the nearest accepted triangle (or -1) and its distance d (MAX_VALUE_DIST = 1e12f on a miss).
 * d_src_idx (may be NULL) gives each ray's idx_source, the triangle to skip (:40-41); NULL means -1 for all.
 * Used by the parity tests to compare scan kernels hit for hit; asynchronous like sphip_render_device. */
int sphip_closest_hit_device(sphip_t* ctx, const void* d_rays, size_t n_rays, const void* d_src_idx /* n_rays i32 or NULL */,
                             int flags, void* d_out_idx /* n_rays i32 */, void* d_out_dist /* n_rays f32 */, void* stream);

/* The row-tile plan, pure host arithmetic (no GPU needed): tiles of `tile_rows` image rows are dealt round-robin, tile t to
 * device t mod n_devices.  sphip_plan_tile_rows: the largest tile height <= 8 that gives every device the same number of
 * whole tiles (8 when none does).  sphip_plan_shard: device `rank`'s sphip_shard and ray count; returns SPHIP_E_INVALID on
 * nonsense arguments. */
int sphip_plan_tile_rows(size_t height, int n_devices);
int sphip_plan_shard(size_t width, size_t height, int n_devices, size_t tile_rows, int rank, sphip_shard* shard_out, size_t* n_rays_out);

/* TEST-ONLY: evaluates one device function of the path for n caller-supplied inputs (host pointers, blocking), so that the
 * device arithmetic can be compared with the oracle directly rather than only through whole renders.
 *   what 0  sincos_glibc   (std::sin/std::cos of geom.h:170-173)   in f32[n]                          out f32[2n] sin, cos
 *        1  recip_ieee     (1.0/a of geom.h:206)                   in f32[n]                          out f32[n]
 *        2  philox_uniforms (replaces frand.h:53-63)               in u32[5n] seed lo, hi, pixel, sample, depth   out f64[2n]
 *        3  rand_unit_vec  (geom.h:164-177, the two draws given)   in f64[5n] n.xyz, r1, r2           out f32[3n]
 *        4  ray_tri_strict (geom.h:197-222)                        in f32[15n] pos dir v0 v1 v2       out f32[n] distance or -1
 *        5  vec3_rgba      (scene.h:32-39)                         in f32[3n]                         out u32[n]
 *        6  the f16 matrix-pipe side product of sp_cylm_scan.h      in f32[12n] 5 triangle values, 5 ray values, P_a (a half), 0
 *                                                                  out f32[2n] the instruction's result, the same 16 products summed in double
 *        7  shade_normal   ("smooth shading" below)                in f32[24n] pos dir v0 v1 v2 n0 n1 n2   out f32[6n] u, v, ns.xyz, sm
 *        8  dielectric     ("transparency" below)                  in f32[8n] dir ns ior entering          out f32[6n] Fr, tir, nt.xyz, c
 *        9  env_lookup     ("environment lighting" below)          in f32[3n] d                            out f32[4n] i, j, r3, valid
 *       10  env_sample     ("environment lighting" below)          in f64[4n] r8 r9 r3 r4                  out f32[6n] i, j, wd.xyz, r3
 *           9 and 10 run against the context's environment map (SPHIP_E_STATE without one)
 *       11  gloss_bounce   ("glossy reflection" below)             in f64[9n] dir.xyz ns.xyz alpha u1 u2 (dir, ns and alpha: f32 values
 *                                                                  carried in doubles, as what 3 does)      out f32[8n] m.xyz, nd.xyz, g, ok
 *       12  tex_albedo     ("textures" below)                      in f32[21n] pos dir v0 v1 v2 uv0 uv1 uv2  out f32[6n] s, t, c.rgb, textured
 *           12 runs against the context's atlas (SPHIP_E_STATE without one); c = 1 where the hit is not textured */
int sphip_selftest_device(sphip_t* ctx, int what, const void* in, size_t n, void* out);

/* TEST-ONLY: stage 1 of the default scan ALONE -- the conservative reject that decides which (ray, triangle) pairs ever reach
 * geom::ray_intersect (src/geom.h:197-222) -- for n_rays host rays (a multiple of 64) against the context's scene, formed
 * exactly as the render kernels form it (same ray setup, same fragment code, same tiles).  A test can then assert, pair by
 * pair, that no pair the reference accepts has its bit clear, instead of observing the filter only through the closest hit.
 *   *tiles_out         bits 0-19: tiles of the scene's stream, bits 20-30: T = triangles per tile, bit 31: one survivor bit per OCTET (two groups
 *                      of four) instead of per group of four (call with out_words = NULL first to size the outputs); W words per ray block
 *                      below: T / 256 with group bits, max(1, T / 512) with octet bits
 *   out_words[((k * tiles + t) * 2 + rb) * W + w]   word w of "lane" k (k = 64 b + l) for tile t.  Group bits: bit 31 - (4 f + j) set = the group of
 *                      four triangles 8 (8 w + f) + 2 j + (l >> 5) of tile t SURVIVES for ray 64 b + (l & 31) + 32 rb (f < 8, j < 4).  Octet bits:
 *                      bit 31 - (2 f + q) set = the groups 8 (16 w + f) + 4 q + (l >> 5) and that + 2 survive (f < 16, q < 2)
 *   out_tri[((k * tiles + t) * 2 + rb) * (T / 64) + f / 2]   (may be NULL) the same side products tested per TRIANGLE with the triangle's own
 *                      cylinder radius (the per-pair form of the test): bit 31 - (16 (f & 1) + 4 j + i) set = triangle
 *                      32 f + 8 j + 4 (l >> 5) + i of tile t survives for that ray (f < T / 32).  Stronger than the group / octet bit: a set
 *                      triangle bit implies the set bit of its group / octet
 *   out_order[t * T + 4 g + u]            index of the triangle at place u of group g of tile t (n_tris = padding; a triangle that
 *                      appears nowhere is in the "big" class: no filter, tested by every ray)
 * Blocking; host pointers; single-device contexts. */
int sphip_selftest_stage1(sphip_t* ctx, const float* rays, size_t n_rays, uint32_t* out_words, uint32_t* out_tri, int32_t* out_order, uint32_t* tiles_out);

/* TEST-ONLY: the RE-TEST of stage 2 of the default scan alone (tests/test_hip_retest_audit.py): for the caller's n_rays rays (a multiple of 64)
 * against EVERY triangle of the scene's stream, whatever stage 1 would say of the pair, the verdict of the f32 cylinder test that decides
 * which triangles of a listed group go on to the exact test -- formed as the render kernels form it: the tile's records (the cylinder of a
 * second edge of the triangle), the same chain, the doubled margin.  No pair the reference accepts may have its bit clear.
 *   *tiles_out         as sphip_selftest_stage1 (call with out_bits = NULL first to size the outputs)
 *   out_bits[(k * tiles + t) * (T / 4) + g]   bit 3 - u set = the triangle at place u of group g of tile t SURVIVES the re-test for ray k
 *   out_order[t * T + 4 g + u]                as sphip_selftest_stage1
 * Blocking; host pointers; single-device contexts.  Additive: the ABI version does not change. */
int sphip_selftest_retest(sphip_t* ctx, const float* rays, size_t n_rays, uint8_t* out_bits, int32_t* out_order, uint32_t* tiles_out);

/* TEST-ONLY: the code underneath the opt-in acceleration structure on its own (tests/test_hip_sort.py, tests/test_hip_bvh_build.py,
 * tests/bvh_checks.py).  Blocking; host pointers; single-device contexts.  Additive: the ABI version does not change.
 *
 * sphip_selftest_sort: the context's own stable radix sort (4-bit digits; the one both the default scan's prepass and the BVH build call)
 * on n caller (key, value) pairs by the low key_bits bits of the key (1..32, rounded up to a whole digit; higher bits are ignored).
 * out_keys / out_vals [n]: the pairs in ascending key order, equal keys in input order.  Needs no scene and disturbs none.
 *
 * sphip_selftest_bvh_dump: builds the linear BVH of the context's scene if it is not built and copies it out.  *n_leaves_out: leaves of the
 * complete tree (a power of two); call with the other outputs NULL first to size them (each may be NULL on its own):
 *   out_meta  u32[16]                      the builder's words: [0..2] scene lo.xyz, [3..5] hi.xyz as ordered uints, [6] / [7] triangles wider than
 *                                          1/4 / 1/2 of the scene, [8] n_big, [9..15] zero
 *   out_nodes f32[2 * n_leaves][8]         heap order (root 1, children 2 i and 2 i + 1, leaf l at n_leaves + l): lo.xyz, hi.xyz, 0, 0; node 0 is
 *                                          never written
 *   out_rec   f32[4 * n_leaves + 256][12]  v0.xyz, e1.xyz, e2.xyz, 0, 0, 0 per slot: four slots per leaf in tree order, then the big list
 *   out_idx   i32[4 * n_leaves + 256]      the slot's triangle, -1 for padding
 *
 * sphip_selftest_bvh_walk: the traversal the render kernels call (scan_bvh) on n_rays caller rays f32[n][6] against the context's scene.
 * src_idx (may be NULL: none) i32[n] the triangle each ray leaves; tmax (may be NULL: unbounded) f32[n] only hits with d < tmax count;
 * any_hit != 0: stop at the first such hit (the shadow form).  out_idx / out_d [n]: the hit, or -1 and the ray's tmax; out_steps [n]:
 * steps of the walk, which ends unfinished when they reach 4 * n_leaves + 64; out_leaves [n]: leaves visited. */
int sphip_selftest_sort(sphip_t* ctx, const uint32_t* keys, const uint32_t* vals, size_t n, uint32_t key_bits, uint32_t* out_keys, uint32_t* out_vals);
int sphip_selftest_bvh_dump(sphip_t* ctx, uint32_t* n_leaves_out, uint32_t* out_meta, float* out_nodes, float* out_rec, int32_t* out_idx);
int sphip_selftest_bvh_walk(sphip_t* ctx, const float* rays, size_t n_rays, const int32_t* src_idx, const float* tmax, int any_hit,
                            int32_t* out_idx, float* out_d, uint32_t* out_steps, uint32_t* out_leaves);

/* ---- progressive rendering: accumulate samples across calls while the view stands still.
 * The counter RNG is keyed by (seed, global pixel, sample index, depth), and samples are added to an f32 sum one at a time in
 * sample order, so after steps of n_1, n_2, ... samples the image (and the mean) is bit-identical to one render of
 * n_1 + n_2 + ... samples: the outputs of every step are what sphip_render returns for the total so far.
 *
 * sphip_render_device_accum: the stateless device-pointer form (single-device contexts; asynchronous like sphip_render_device;
 * path tracing only).  Renders global samples [sample_base, sample_base + n_samples) of the shard's rays into the running sum
 * d_sum (n_rays*3 f32, AoS: the raw sum, not the mean; in place).  sample_base == 0 ignores d_sum's contents (no clearing
 * needed).  d_out_rgba / d_out_mean (may be NULL) receive the image and the mean of all sample_base + n_samples samples.
 * sample_base + n_samples must stay below 2^31. */
int sphip_render_device_accum(sphip_t* ctx, const void* d_rays /* n_rays*6 f32 */, size_t n_rays, const sphip_shard* shard /* NULL = whole */,
                              size_t image_width, uint64_t sample_base, size_t n_samples, uint64_t seed, int flags,
                              void* d_sum /* n_rays*3 f32, in/out */, void* d_out_rgba /* n_rays*4 u8 */, void* d_out_mean /* n_rays*3 f32 or NULL */,
                              void* stream);
/* sphip_accum_begin: starts an accumulation of the w*h viewport given by exactly one of `rays` (host array, w*h*6 f32, uploaded
 * once) and `cam` (generated on the device; cam->res_x/res_y must equal w/h).  The rays and the running sum live in buffers of
 * the accumulation: sphip_render / sphip_render_camera calls in between do not disturb it.  Needs a scene (SPHIP_E_STATE).
 * Accepted by multi-device contexts: every device keeps the rays and the sum of its row tiles resident.
 * sphip_accum_step: n_samples more samples; blocking, host outputs like sphip_render (out_mean may be NULL); *total_out (may be
 * NULL) = samples accumulated so far.  sphip_get_stats then describes this step.  SPHIP_E_STATE when no accumulation was begun
 * or a scene has been set since the begin; SPHIP_E_INVALID for n_samples == 0 or a total reaching 2^31.  A step that fails on
 * the device ends the accumulation (begin again). */
int sphip_accum_begin(sphip_t* ctx, const float* rays /* w*h*6 f32 or NULL */, const sphip_camera* cam /* or NULL */,
                      size_t w, size_t h, uint64_t seed, int flags);
int sphip_accum_step(sphip_t* ctx, size_t n_samples, uint8_t* out_rgba /* w*h*4 */, float* out_mean /* w*h*3 or NULL */,
                     uint64_t* total_out /* or NULL */);

/* ---- adaptive sampling: a progressive accumulation that stops converged pixels.
 * Every pixel starts active.  A step (sphip_accum_step) of n samples renders global samples [total, total + n) for the active
 * pixels only (they all share the count `total`).  Per sample and pixel the library keeps, in double and in sample order,
 * y = ((double)r + (double)g) + (double)b of the sample's f32 radiance, S1 += y and S2 += y * y.  After the step each pixel still
 * active with count n >= min_samples is tested, in double, in this order:
 *     m = S1 / n;  v = (S2 - S1 * m) / (n - 1);  r = m > floor ? m : floor;  d = rel_error * r;  stop iff v / n <= d * d
 * A stopped pixel never restarts; its sum, S1, S2 and count stay frozen.  Every step returns the whole frame, each pixel from
 * its own sum and count, so a pixel that stopped after n samples holds exactly what sphip_render of n samples gives for it.
 * Decisions are taken at step ends only: the counts depend on how the samples are split into steps, not on the kernel
 * variant, sample chunks, primary-hit reuse, SPHIP_FLAG_ACCEL, sharding or the number of devices.
 * sphip_accum_step then sets *total_out to the count of the still-active pixels; a step with no active pixel renders nothing,
 * returns the unchanged image, executes 0 scans and does not advance the total.  sphip_get_stats describes the step
 * (scans_executed: the scans actually run). */
typedef struct {
	double   rel_error;    /* t >= 0 (finite) */
	double   floor;        /* f >= 0 (finite): the mean below which the error is measured absolutely */
	uint32_t min_samples;  /* >= 2: no pixel stops before this many samples */
	uint32_t reserved;     /* must be 0 */
} sphip_adaptive;

/* sphip_accum_begin plus the rule (same rays / camera, seed, flags, reset rules and error contract); SPHIP_E_INVALID for a
 * NULL a, min_samples < 2, a negative or non-finite rel_error or floor, reserved != 0.  Accepted by multi-device contexts:
 * every device runs the rule on its own row tiles. */
int sphip_accum_begin_adaptive(sphip_t* ctx, const float* rays /* w*h*6 f32 or NULL */, const sphip_camera* cam /* or NULL */,
                               size_t w, size_t h, uint64_t seed, int flags, const sphip_adaptive* a);
/* Per-pixel sample counts of the current accumulation in image order (out_counts may be NULL) and the number of active
 * pixels (may be NULL).  A plain accumulation reports `total` for every pixel, all of them active.  Blocking; SPHIP_E_STATE
 * when no accumulation has been begun. */
int sphip_accum_counts(sphip_t* ctx, uint32_t* out_counts /* w*h or NULL */, uint64_t* n_active_out /* or NULL */);

/* ---- denoising: an edge-aware a-trous wavelet filter (Dammertz et al. 2010) with SVGF-style variance guidance, guided by a
 * noise-free G-buffer of the primary hits.  A post-process: it leaves the scans, the sums and the raw
 * image as they are.  Every operation is an f32 + - * / (IEEE division), a comparison or a select in the order below, so the
 * output is reproducible bit for bit; max(0, x) means x > 0 ? x : 0.
 *
 * G-buffer: 32 B per pixel {f32 nx, ny, nz, dist; f32 ar, ag, ab; i32 mat}, from the pixel's primary ray (idx_source = -1) and
 * the closest hit sphip_closest_hit_device returns for the same rays and flags (SPHIP_FLAG_ACCEL included).  Hit: n = the
 * triangle's normal, negated when dot3(n, dir) > 0; dist = the hit distance; a = the triangle's reflectance; mat = the smallest
 * triangle index whose 6 material floats are bitwise equal to the hit triangle's (derived once per scene).  Miss: n = 0,
 * dist = 1e12f, a = 0, mat = -1.
 *
 * Filter: iterations i = 0 .. K-1 with step s = 2^i, each on an f32 {r, g, b, var} per pixel.  A miss pixel (mat_p = -1)
 * passes through.  For any other pixel p the taps q = p + s * (dx, dy) are visited dy, then dx, over -2 .. 2; taps outside the
 * image are skipped.  The centre tap has w = 9/64.  Any other tap with mat_q != mat_p is skipped; else
 *     d  = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z;  wn = max(0, d), then normal_log2 times wn = wn * wn
 *     dd = |dist_p - dist_q|;  zd = (sigma_depth * s) * dist_p;  wz = zd == 0 ? (dd == 0) : max(0, 1 - dd / zd)
 *     l  = (r + g) + b of this iteration's input;  dl = l_p - l_q;  ld = (sigma_lum * sigma_lum) * var_p
 *     wl = 1 without variance or when var_p = +inf;  else ld == 0 ? (dl == 0) : max(0, 1 - (dl * dl) / ld)
 *     w  = (((h[dx] * h[dy]) * wn) * wz) * wl,  h = {1/16, 1/4, 3/8, 1/4, 1/16}
 * A tap counts only when ww = w * w > 0: W += w; C.rgb += w * c_q.rgb (per channel); V += ww * var_q (sums start at 0).
 * Output of the iteration: rgb = C / W per channel, var = V / (W * W).  Final output: the rgb of the last iteration and its
 * RGBA8 through vec3::clamp and scene::vec3_RGBA (as the render's).  K = 0: the input itself. */
typedef struct {
	uint32_t iterations;   /* K, 0..8 */
	uint32_t normal_log2;  /* 0..8 */
	float    sigma_depth;  /* > 0, finite */
	float    sigma_lum;    /* > 0, finite */
	uint32_t reserved[2];  /* must be 0 */
} sphip_denoise;

/* the calibrated defaults */
void sphip_denoise_defaults(sphip_denoise* out);
/* G-buffer of n_rays primary rays (device pointers, d_out_gbuf n_rays * 32 B); asynchronous like sphip_closest_hit_device, single-device
 * contexts (SPHIP_E_STATE otherwise).  The first call after a scene change reads the materials back once (material classes). */
int  sphip_gbuffer_device(sphip_t* ctx, const void* d_rays, size_t n_rays, int flags, void* d_out_gbuf, void* stream);
/* The filter on a w*h image: d_mean w*h*3 f32, d_var w*h f32 or NULL (no luminance weight), d_gbuf from sphip_gbuffer_device of the
 * image's rays; d_out_rgba w*h*4 u8, d_out_rgb w*h*3 f32 or NULL.  Asynchronous; single-device contexts (SPHIP_E_STATE otherwise). */
int  sphip_denoise_device(sphip_t* ctx, const sphip_denoise* p, size_t w, size_t h, const void* d_mean, const void* d_var, const void* d_gbuf,
                          void* d_out_rgba, void* d_out_rgb, void* stream);
/* The current accumulation's G-buffer (host output, w*h*32 B), built with the accumulation's flags and cached until the next begin.
 * Blocking; SPHIP_E_STATE with no accumulation or after a set_scene since the begin. */
int  sphip_accum_gbuffer(sphip_t* ctx, void* out_gbuf);
/* Denoises the current accumulation without altering it: the mean of every pixel (its sum times float(1.0 / count)) and, for an
 * adaptive accumulation, the variance of that mean: per pixel, in double, with the rule's m and v, (float)max(0, v / n), +inf
 * when n < 2.  A plain accumulation has no statistics and is filtered without wl.  Builds and caches the G-buffer on first use.
 * Blocking; host outputs (out_rgb may be NULL).  sphip_get_stats then describes the call: the filter's kernels, plus the G-buffer
 * scan (scans_executed = w*h) when the call built it.  SPHIP_E_STATE before the first step or after a set_scene since the begin.
 * Multi-device contexts are accepted and give the single-device bytes: every device prepares its row tiles, the frame is
 * filtered on the first device. */
int  sphip_accum_denoise(sphip_t* ctx, const sphip_denoise* p, uint8_t* out_rgba, float* out_rgb /* or NULL */);

/* ---- temporal reprojection: the step SVGF-style pipelines put in front of the a-trous filter.  When the camera
 * moves, the previous view's accumulated radiance (a mean and a per-pixel history count: how many samples the mean stands for) is
 * resampled at the new view's primary hits and blended with the new view's samples, so that an accumulation survives the move.  A
 * post-process like the denoiser: it leaves the scans, the sums and every render as they are.  Every operation is an f32 + - * /
 * (IEEE division), a comparison, a select or a float-to-int floor in the order below, nothing fused, so the output is reproducible bit
 * for bit; dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z.
 *
 * Inputs: the current view's rays and G-buffer (sphip_viewport_device of the new camera, sphip_gbuffer_device of those rays), the
 * previous view's rays, G-buffer, mean and history count, and the previous camera `prev`.  Host constants of `prev`, formed exactly as
 * sphip_viewport_device forms them (src/view.h:101-108): x_max, x_step, h_x, y_max, y_step, h_y; xo = x_max - h_x, yo = y_max - h_y (f32).
 *
 * Reprojection of the current pixel p = y * w + x, G-buffer entry (n_p, dist_p, mat_p), primary ray (o_p, d_p):
 *   1. mat_p < 0 (a miss): mean 0, history 0.
 *   2. P = o_p + d_p * dist_p per component (one multiply, one add).
 *   3. v = P - prev.pos per component.  The inverse of rel_move (src/view.h:54-68,83-85: rel_move = rY(rX(.))), rY's first:
 *        a = (v.x * cos_y + v.z * -sin_y,  v.y,  v.x * sin_y + v.z * cos_y)
 *        c = (a.x,  a.y * cos_x + a.z * sin_x,  a.y * -sin_x + a.z * cos_x)
 *      The reference's rays leave the view plane z = 0 towards (px, py, focal): the eye is (0, 0, -focal).  No history unless c.z > 0.
 *        qz = c.z + focal;  sx = (c.x * focal) / qz;  sy = (c.y * focal) / qz
 *   4. fx = (xo - sx) / x_step;  fy = (yo - sy) / y_step  (the inverse of src/view.h:111).  No history when fx or fy is not finite.
 *      x0 = floor(fx);  tx = fx - x0;  ux = 1 - tx;  y0, ty, uy likewise.
 *   5. The taps q = (x0 + a, y0 + b), visited b, then a, over {0, 1}; wb = (a ? tx : ux) * (b ? ty : uy).  A tap counts only when all of
 *      these hold, tested in this order (nothing of a tap is read before the first):
 *        0 <= x0 + a < w and 0 <= y0 + b < h;   wb > 0;   hist_q > 0;   mat_q == mat_p;   dot3(n_p, n_q) >= normal_min;
 *        |dot3(P_q - P, n_p)| <= plane_tol * dist_p,  P_q = o_q + d_q * dist_q of the PREVIOUS view's ray and G-buffer entry q
 *   6. Sums from 0, in tap order:  W += wb;  C.rgb += wb * mean_q.rgb (per channel);  Hs += wb * hist_q.
 *      !(W > 0): mean 0, history 0.  Else mean = C / W per channel;  hist = Hs / W;  hist = hist > max_history ? max_history : hist.
 *
 * Blend of a history (hm, h) with the running sum s of n new samples, per channel:
 *      h == 0:  s * (float)(1.0 / n)  -- what every render and accumulation step writes, so a pixel without history is bit for bit the
 *               plain accumulation's;   else  (h * hm + s) / (h + (float)n)
 * RGBA8 through vec3::clamp and scene::vec3_RGBA, as the render's.  The history that a blended accumulation of n samples hands to the
 * next reprojection is (that blend, h + (float)n); the cap max_history applies in step 6 alone.
 *
 * What it is not: the history is an unbiased estimate of the new pixel only where the first hit is diffuse.  Mirrors, glass, glossy
 * highlights and depth of field depend on the view and lag by up to max_history samples; the bilinear resampling blurs across
 * irradiance gradients.  There is no per-material rejection. */
typedef struct {
	float    max_history;   /* >= 0, finite: cap of the per-pixel history count (0: no history is taken over) */
	float    normal_min;    /* in [-1, 1]: a tap counts only when dot3(n_p, n_q) >= normal_min */
	float    plane_tol;     /* >= 0, finite: a tap counts only when |dot3(P_q - P, n_p)| <= plane_tol * dist_p */
	uint32_t reserved;      /* must be 0 */
} sphip_reproject;

/* the calibrated defaults */
void sphip_reproject_defaults(sphip_reproject* out);
/* Steps 1-6 for the w*h pixels of the current view.  Device pointers: rays w*h*6 f32, G-buffers w*h*32 B (16-byte aligned),
 * d_mean_prev / d_out_mean w*h*3 f32, d_hist_prev / d_out_hist w*h f32; the outputs overlap no input.  Stateless; needs no scene;
 * asynchronous on `stream`; single-device contexts (SPHIP_E_STATE otherwise).  SPHIP_E_INVALID: a NULL pointer, w or h 0 or >= 2^30,
 * cam_prev->res_x/res_y differing from w/h, a parameter out of its range or not finite, reserved != 0. */
int sphip_reproject_device(sphip_t* ctx, const sphip_reproject* p, const sphip_camera* cam_prev, size_t w, size_t h,
                           const void* d_rays_cur, const void* d_gbuf_cur, const void* d_rays_prev, const void* d_gbuf_prev,
                           const void* d_mean_prev, const void* d_hist_prev, void* d_out_mean, void* d_out_hist, void* stream);
/* The blend for n pixels: d_sum n*3 f32 (the raw sum of n_samples > 0 samples, as sphip_render_device_accum keeps it), d_hist_mean n*3 f32
 * and d_hist n f32 (both NULL: no pixel has a history); d_out_rgba n*4 u8 and d_out_mean n*3 f32, either may be NULL, not both.
 * Stateless, asynchronous, single-device contexts like the call above. */
int sphip_temporal_resolve_device(sphip_t* ctx, size_t n, const void* d_sum, uint32_t n_samples, const void* d_hist_mean, const void* d_hist,
                                  void* d_out_rgba, void* d_out_mean, void* stream);
/* Moves the current accumulation to the view cam_new and keeps what it has gathered as history.  Needs a live accumulation that was
 * begun with `cam` (not rays), is plain (not adaptive), lives on a single-device context and has taken at least one step.  The call
 * turns that accumulation (with its own history, if it has one) into a (mean, history count) pair, reuses the old view's cached
 * G-buffer (building it if no call has yet), generates the new view's rays and G-buffer, reprojects, and begins a new accumulation for
 * cam_new with the old flags and lens and the given seed, with the reprojected history attached.  After it sphip_accum_step returns
 * the blend (*total_out counts the new samples only), sphip_accum_denoise filters the blended mean (without wl, as for any plain
 * accumulation), sphip_accum_gbuffer is the new view's, and the call may be repeated any number of times.  sphip_accum_begin and
 * sphip_accum_begin_adaptive drop the history.  Pass a seed other than the history's: the same seed at the same view draws the same
 * samples again, which adds nothing.  Blocking.
 * A refusal changes nothing (the next step is what it would have been).  SPHIP_E_STATE: no accumulation, one ended by a setter or a
 * set_scene, one begun with rays, an adaptive one, a multi-device context, or before the first step.  SPHIP_E_INVALID: a NULL
 * argument, cam_new->res_x/res_y differing from the accumulation's, a parameter out of its range or not finite, reserved != 0.
 * A call that fails on the device (SPHIP_E_DEVICE) ends the accumulation, as a failing step does (begin again). */
int sphip_accum_reproject(sphip_t* ctx, const sphip_camera* cam_new, uint64_t seed, const sphip_reproject* p);
/* The per-pixel history counts of the current accumulation in image order (all 0 for one without history).  Blocking; SPHIP_E_STATE when
 * no accumulation has been begun. */
int sphip_accum_history(sphip_t* ctx, float* out_hist /* w*h */);

/* ---- display transform: the last stage of the viewer pipeline.  Every render, step, denoise and blend above
 * ends in vec3::clamp and scene::vec3_RGBA: a linear clamp to [0, 1] and * 255 + 0.5, which is the reference's and right for its closed
 * room, and which shows an HDR sky, a small bright emitter or a lamp as a white sheet.  This stage turns a mean image (f32 rgb radiance)
 * into pixels the way a viewer expects: an exposure (given, or metered from the image), a tone curve, then the linear or the sRGB
 * encoding.  A post-process over the mean: it touches no scan, no integrator and no sum.  On the device every operation is an f32
 * + - * / (IEEE division), a comparison, a select, a bit cast or an integer operation in the order below, nothing fused, so the output is
 * reproducible bit for bit; bits(x) is the f32's bit pattern as a u32.
 *
 * Luminance:  lum(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b
 *
 * Histogram (metering): 2048 u32 bins over the pixels of the mean.  With l = lum(c): a pixel with !(l > 0) (zero, negative, NaN) counts in
 * bin 0, any other in bin bits(l) >> 20 (+inf: bin 2040).  The bin is the f32 exponent and the top three mantissa bits: a logarithmic
 * histogram, eight bins per octave, without a transcendental function; a sum of integers, the same in whatever order it is formed.
 *
 * Exposure from a histogram: host arithmetic in double, in this order.  The valid bins are b = 8 .. 2039 (bin 0, the denormals' bins 1 .. 7
 * and infinity's are ignored), and a valid bin stands for the level
 *     L[b] = (double)((int)(b >> 3) - 127) + ((double)(b & 7) + 0.5) / 8.0
 * the piecewise-linear (Mitchell) log2 of the bin's centre, exact in double.  N = the pixels in valid bins; N == 0: exposure 1.
 *     lo = (u64)((double)low * (double)N);   hi = N - (u64)((1.0 - (double)high) * (double)N);   hi <= lo: lo = 0, hi = N
 * The valid pixels are ranked 0 .. N-1 in ascending bin order; bins in ascending order, `part` = the number of the bin's pixels whose rank
 * lies in [lo, hi):  M += part;  S += (double)part * L[b]  (M a u64, S a double from 0.0).  Then
 *     mean = S / (double)M;   x = -mean clamped to [-126, 126];   f = floor(x);   E = (float)((double)key * ldexp(1.0 + (x - f), (int)f))
 * ldexp of 1 + frac is the exact inverse of L, so no log2 or exp2 of any libm is called.  The metered level lies within Mitchell's
 * 0.086 of a true log-average (about 6 % in exposure).
 *
 * Transform of a pixel c with exposure E:  v = c * E per channel, then the curve
 *     SPHIP_CURVE_CLAMP     v
 *     SPHIP_CURVE_REINHARD  extended Reinhard on luminance with white point w:  l = lum(v);  !(l > 0): v;  else
 *                           s = (1.0f + l / (w * w)) / (1.0f + l);  v = v * s per channel  (l = w maps to luminance 1, up to rounding)
 *     SPHIP_CURVE_FILMIC    Narkowicz's fit of the ACES curve, per channel x:
 *                           (x * ((2.51f * x) + 0.03f)) / ((x * ((2.43f * x) + 0.59f)) + 0.14f)
 * then vec3::clamp (x > 1 ? 1 : (x < 0 ? 0 : x), which lets a NaN through): this triple is the float output, display-linear.  Then
 *     SPHIP_ENCODE_LINEAR   scene::vec3_RGBA, as every render
 *     SPHIP_ENCODE_SRGB     the code of a channel x = the number of k in 1 .. 255 with x >= T[k] (an 8-step binary search; a NaN is 0),
 *                           T[k] = the f32 nearest to the inverse sRGB transfer function at (k - 0.5) / 255.  The 255 values are literals
 *                           (spath_amd/csrc/sp_srgb_table.h, sphip_srgb_thresholds): the table is the contract, no pow is evaluated
 * Alpha is 0.  A non-finite input goes where IEEE arithmetic takes it (inf / inf is a NaN under either curve, shown as 0).
 * With E = 1, SPHIP_CURVE_CLAMP and SPHIP_ENCODE_LINEAR the RGBA8 is, bit for bit, what every render and step writes for that mean. */
enum { SPHIP_CURVE_CLAMP = 0, SPHIP_CURVE_REINHARD = 1, SPHIP_CURVE_FILMIC = 2 };
enum { SPHIP_ENCODE_LINEAR = 0, SPHIP_ENCODE_SRGB = 1 };
typedef struct {
	float    exposure;     /* > 0, finite: E when the call does not meter */
	float    white;        /* > 0, finite: Reinhard's white point w (read by that curve only) */
	uint32_t curve;        /* SPHIP_CURVE_* */
	uint32_t encode;       /* SPHIP_ENCODE_* */
	uint32_t reserved[2];  /* must be 0 */
} sphip_display;
typedef struct {
	float    key;          /* > 0, finite: the level the metered log-average is mapped to */
	float    low, high;    /* 0 <= low < high <= 1: the rank window, as fractions of the valid pixels */
	uint32_t reserved;     /* must be 0 */
} sphip_metering;

/* curve FILMIC, encode SRGB, exposure 1, white 4; key 0.18, low 0.5, high 0.95: conventions, not measurements */
void sphip_display_defaults(sphip_display* out);
void sphip_metering_defaults(sphip_metering* out);
/* T[1] .. T[255] into out[0] .. out[254]; needs no GPU */
void sphip_srgb_thresholds(float out[255]);
/* The histogram of the n pixels of d_mean (n*3 f32) into d_out_hist (2048 u32; zeroed by the call on the same stream).  Device pointers;
 * stateless; needs no scene; asynchronous on `stream`; single-device contexts (SPHIP_E_STATE otherwise).  SPHIP_E_INVALID: a NULL
 * pointer, n == 0 or n >= 2^32. */
int  sphip_luminance_histogram_device(sphip_t* ctx, size_t n, const void* d_mean, void* d_out_hist /* 2048 u32 */, void* stream);
/* "Exposure from a histogram" above for a host copy of the 2048 bins.  Host only, no context, no GPU.  SPHIP_E_INVALID (*exposure_out
 * untouched): a NULL pointer, key not finite or not > 0, low or high outside [0, 1], low >= high, reserved != 0. */
int  sphip_exposure_from_histogram(const uint32_t* hist, const sphip_metering* m, float* exposure_out);
/* The transform of the n pixels of d_mean with E = p->exposure: d_out_rgba n*4 u8, d_out_rgb n*3 f32 or NULL; the outputs overlap no
 * input.  Pointers that are all 16-byte aligned move four pixels per lane as whole vectors; any alignment gives the same bytes.
 * Stateless, asynchronous, single-device contexts like the histogram.  SPHIP_E_INVALID: a NULL p, d_mean or d_out_rgba, n == 0 or
 * n >= 2^32, exposure or white not finite or not > 0, an unknown curve or encoding, reserved != 0. */
int  sphip_display_device(sphip_t* ctx, const sphip_display* p, size_t n, const void* d_mean, void* d_out_rgba, void* d_out_rgb /* or NULL */,
                          void* stream);
/* Shows the current accumulation without altering it.  The input is the mean sphip_accum_step would return -- plain, adaptive (each
 * pixel from its own count) or blended with a history after sphip_accum_reproject -- or, with dn, the output of sphip_accum_denoise(dn)
 * (which builds and caches the G-buffer on first use, as that call does; without dn no G-buffer is built or read).  With m that image
 * is metered first and E is the metered exposure; without, p->exposure.  *exposure_out (may be NULL) = the E that was used.  Blocking;
 * host outputs (out_rgb may be NULL: the display-linear float).  Multi-device contexts are accepted as by sphip_accum_denoise, with the
 * bytes of one device.  A refusal changes nothing.  SPHIP_E_INVALID: a NULL p or out_rgba, a bad *p, *m or *dn (as the calls above and
 * sphip_accum_denoise refuse them).  SPHIP_E_STATE: exactly where sphip_accum_denoise returns it. */
int  sphip_accum_display(sphip_t* ctx, const sphip_display* p, const sphip_metering* m /* NULL: p->exposure as given */,
                         const sphip_denoise* dn /* NULL: the raw mean */, uint8_t* out_rgba, float* out_rgb /* or NULL */,
                         float* exposure_out /* or NULL */);

/* ---- next-event estimation (SPHIP_FLAG_NEE): at each of the first four surface hits of a path, one light
 * sample and one shadow ray.  Valid for SPHIP_MODE_PT on every render and accumulation entry point and with the variants 1,
 * 2, 8 (SPHIP_FLAG_ACCEL), 15 and 16, every one the library carries (a retired number is SPHIP_E_INVALID with or without the flag); flat and hit queries ignore it.
 * Every operation below is f32 unless marked double; dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z.
 *
 * Paths: the same closest hits and BSDF directions as without the flag (philox_uniforms(seed, pixel, sample, depth)), but at most
 * four hits: the fifth would carry nothing.  Radiance, unwound from the last hit (rec = 0 beyond it):
 *     rec_d = (e_d + L_d) + (((brdf_d * rec_{d+1}) * ct_d) * (1/p)),   e_0 = the first hit's emittance, e_d = 0 for d >= 1
 * (brdf_d = reflectance * (1/pi) and ct_d as without the flag; per channel, in this order).
 *
 * Light table (once per scene, on the first NEE render after a set_scene; a negative or non-finite emittance component anywhere in
 * the scene makes every NEE render fail with SPHIP_E_INVALID): the triangles with Esum = ((double)Er + Eg) + Eb > 0 and
 * w = A * Esum > 0, in ascending index, A = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz) in double of c = e1 x e2, e1 = (double)v1 -
 * (double)v0, e2 = (double)v2 - (double)v0; cdf = their running double sum, W = its last entry, ipdf = (float)(W / Esum).
 * No entry: L_d = 0 everywhere.
 *
 * Light sample at hit d (point x = o + dir * dist of the hit, triangle src, normal n turned against dir as the path uses it):
 *     (r3, r4) = philox_uniforms(seed, pixel, sample, 8 + d);  r5 = the first draw of philox_uniforms(seed, pixel, sample, 16 + d)
 *     e = the first entry with cdf > r5 * W (double), the last entry if none;  i = its triangle
 *     a = (float)sqrt(r3) (double sqrt);  b = (float)r4;  y = (v0 + e1 * (a * (1 - b))) + e2 * (a * b)   (e1 = v1 - v0, e2 = v2 - v0)
 *     w = y - x;  dist2 = dot3(w, w);  dist = sqrtf(dist2);  wd = w / dist (per component)
 *     cos_x = dot3(wd, n);  cos_y = |dot3(wd, n_i)|   (n_i: triangle i's normal; emitters are two-sided);  sxz = sqrtf(wd.x * wd.x + wd.z * wd.z)
 *     L_d = 0 without a shadow ray when i == src, !(dist2 > 0), !(cos_x > 0), !(cos_y > 0) or !(sxz > 0);  else the shadow ray
 *     (x, wd) skips src with tmax = dist * (1 - 2^-10), and L_d = 0 when it is occluded, else
 *     L_d = (reflectance_src * (1/pi)) * (Le_i * ((((cos_x * cos_y) / dist2) * ipdf_e) * ((float)(2/pi) / sxz)))   (per channel)
 * The last factor is 2 pi times the density per solid angle of the reference's BSDF directions (geom.h:164-177 draws the elevation
 * above the world y plane uniformly in angle: 1 / (pi^2 sqrt(x^2 + z^2))), so that NEE estimates the plain estimator's image.
 * Occluded: some triangle other than src gives 0 < d < tmax under the reference's strict triangle test, i.e. the closest hit that
 * skips src (sphip_closest_hit_device) lies below tmax.  Every scan variant agrees on it bit for bit.
 * sphip_stats.scans_executed counts the path scans plus the shadow rays traced (one each, whether the scan left early or not).
 * Progressive and adaptive accumulation (the luminance proxy of the NEE sample), primary-hit reuse, sample chunks, denoising,
 * shards and multi-device contexts work as without the flag, bit for bit. */

/* ---- multiple importance sampling (SPHIP_FLAG_MIS | SPHIP_FLAG_NEE): next-event estimation's light samples at
 * hits 0..3 and the emission that BSDF directions find at hits 1..4, combined by the balance heuristic.  Valid wherever
 * SPHIP_FLAG_NEE is; SPHIP_FLAG_MIS without SPHIP_FLAG_NEE makes a path-traced render fail with SPHIP_E_INVALID (flat and hit queries
 * ignore both).  Notation, light table, draws and shadow rays as for next-event estimation above.
 *
 * Paths: the same closest hits and BSDF directions, up to five hits (the fifth is traced again: its emission counts).  Radiance:
 *     rec_d = D_d + (((brdf_d * rec_{d+1}) * ct_d) * (1/p)),   D_d = Ew_d + L_d (d = 0..3),  D_4 = Ew_4   (per channel)
 * u (both densities per solid angle: p_l = dist2 / (cos_y * ipdf) of the light table, q = 1 / (pi^2 sxz) of the BSDF directions):
 *     u(sxz, dist2, cos_y, ipdf) = (((float)(pi^2) * sxz) * dist2) / (cos_y * ipdf),   0 where that quotient is NaN (0/0, inf/inf)
 * Ew_d, the emission e_d = Le of the triangle j hit at depth d:  Ew_0 = e_0;  for d >= 1, with tipdf[j] = ipdf of j's table entry or
 * 0 when j is not in the table (no emittance, zero area, empty table):  Ew_d = e_d when !(tipdf[j] > 0), else Ew_d = e_d / (1 + u_b)
 * per channel, u_b = u(sqrtf(dir.x * dir.x + dir.z * dir.z), bd * bd, |dot3(dir, n_j)|, tipdf[j]), where dir is the BSDF direction
 * (the ray of depth d), bd its closest-hit distance and n_j triangle j's stored normal.
 * Light sample at hit d (d = 0..3): as for next-event estimation except that sxz = 0 is no early-out (the term stays finite), and
 *     L_d = (reflectance_src * (1/pi)) * (Le_i * (((float)(2 pi) * cos_x) / (1 + u(sxz, dist2, cos_y, ipdf_e))))   (per channel)
 * -- NEE's term times u / (1 + u), with the 1/dist2 and 1/sxz factors cancelled, so it never exceeds 2 * reflectance * Le.
 * L_d = 0 where NEE's would be (no sample, or occluded).  A sample's radiance is therefore at most
 * sum_{d=0..4} (2 rho_max)^d (Le_max + 2 rho_max Le_max) per channel.  scans_executed: path scans plus shadow rays.  The image and
 * every composition are bit-for-bit as for next-event estimation (the luminance proxy is that of the MIS sample). */

/* ---- camera samples (SPHIP_FLAG_CAMERA_SAMPLES): every (pixel, sample) of a path-traced render that has a camera
 * starts from a primary ray of its own, generated on the device inside the path-tracing kernels: a box-filtered position in the pixel
 * and, when the lens has a nonzero aperture, a point on a thin lens.  Without the flag every sample starts from the pixel-centre ray of
 * sphip_viewport_device (src/cpu_renderer.cpp:74-76 with src/view.h:111).
 *
 * Valid on sphip_render_camera and on sphip_accum_begin / sphip_accum_begin_adaptive with `cam` (multi-device contexts included), with
 * sample chunks, SPHIP_FLAG_NEE and SPHIP_FLAG_MIS, and with the shipped variants 1, 2, 8 (SPHIP_FLAG_ACCEL), 15 and 16.
 * SPHIP_E_INVALID: on a path that takes rays (sphip_render, sphip_render_device, sphip_render_device_accum, sphip_accum_begin with
 * rays), together with SPHIP_FLAG_PRIMARY_REUSE, with any other variant.  Flat mode and hit queries ignore the flag; the G-buffer of
 * an accumulation stays that of the pixel-centre rays.  sphip_stats.scans_executed keeps its meaning.
 *
 * Arithmetic, with the constants x_max, x_step, y_max, y_step, focal, the rotation and pos of sphip_viewport_device (src/view.h:101-108),
 * global pixel p, i = p % res_x, j = p / res_x, global sample s; f32 unless marked double, nothing fused, dot3 as for NEE below:
 *     (r1, r2) = philox_uniforms(seed, p, s, 24)
 *     cur = ((x_max - x_step * (float)i) - x_step * (float)r1, (y_max - y_step * (float)j) - y_step * (float)r2, 0);  t = cur + (0, 0, focal)
 *     aperture == 0:  o = cur;  g = t
 *     aperture  > 0:  (r3, r4) = philox_uniforms(seed, p, s, 25);  rho = aperture * (float)sqrt(r3) (double sqrt);
 *                     phi = (float)((r4 * pi) * 2.0) (double, as geom.h:167);  (sn, cs) = sincos_glibc(phi) (selftest what 0)
 *                     o = (cur.x + rho * cs, cur.y + rho * sn, 0);  k = focus_dist / focal;  F = cur + t * k (per component);  g = F - o
 *     l = sqrtf(dot3(g, g));  dir = rel_move(g / l per component);  pos = rel_move(o) + cam.pos   (rel_move: src/view.h:83-85)
 * i.e. the reference camera with its lens on the image plane; the plane in focus is local z = focus_dist.  With aperture 0 the ray is
 * sphip_viewport_device's pinhole ray at the jittered position.  Draw keys 24 and 25 are disjoint from the path's (0..4, 8..11, 16..19). */
typedef struct {
	float    aperture;     /* >= 0, finite: radius of the lens disk on the image plane (the image is 1 unit high); 0 = pinhole */
	float    focus_dist;   /* > 0, finite when aperture > 0: local z of the plane in focus */
	uint32_t reserved;     /* must be 0 */
} sphip_lens;

/* The context's lens (NULL = aperture 0), for its later camera-sample renders.  An accumulation captures the lens at its begin: a later
 * sphip_set_lens applies from the next begin.  SPHIP_E_INVALID for a negative or non-finite aperture, a focus_dist that is not finite and
 * positive when aperture > 0, reserved != 0.  Accepted by multi-device contexts. */
int sphip_set_lens(sphip_t* ctx, const sphip_lens* lens);
/* The res_x*res_y primary rays of global sample `sample` with the context's lens (d_rays_out: res_x*res_y*6 f32, ray k = pixel k), from
 * the device function the kernels call; asynchronous, single-device contexts (SPHIP_E_STATE otherwise).  A chain of one-sample
 * sphip_render_device_accum calls (sample_base = s) over these rays gives a flagged render's image bit for bit. */
int sphip_camera_rays_device(sphip_t* ctx, const sphip_camera* cam, uint64_t seed, uint32_t sample, void* d_rays_out, void* stream);

/* ---- specular reflection (SPHIP_FLAG_SPECULAR): a per-triangle specular table beside the scene's materials,
 * 4 f32 per triangle: ks.r, ks.g, ks.b, p.  ks is the mirror reflectance per channel, p the probability that a hit on the triangle
 * takes the mirror lobe: p = 0 leaves the triangle as it is without the table, p = 1 makes it a pure mirror, in between one sample
 * takes one lobe.  The 6-float material and sphip_set_scene are unchanged.
 *
 * Valid for SPHIP_MODE_PT with the plain estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS, with the shipped variants 1, 2, 8
 * (SPHIP_FLAG_ACCEL), 15 and 16, with progressive and adaptive accumulation, sphip_accum_denoise (the G-buffer is unchanged: the lobe
 * is chosen per sample), sample chunks, primary-hit reuse (the shared primary hit stays valid), SPHIP_FLAG_CAMERA_SAMPLES and
 * multi-device contexts.  SPHIP_E_INVALID: with SPHIP_MODE_FLAT; with any other variant; with SPHIP_FLAG_NEE without SPHIP_FLAG_MIS
 * (plain NEE stops after four hits because the fifth carries nothing, which a mirror at hit 3 breaks, and it is the firefly-prone
 * estimator MIS replaced: leaving it out saves a third of the specular kernels).  SPHIP_E_STATE: the flag without a table.  Hit queries
 * ignore the flag.  Without the flag every render is bit for bit what it is without a table; with the flag and a table of zeros too.
 *
 * The estimator, at hit d (d = 0..4) of the path of (seed, global pixel, global sample) on triangle i, (ks, p) = spec[i], n the
 * triangle's normal turned against dir as always, (r1, r2) the direction draws of Philox stream d as always; f32, every operation
 * rounded on its own, nothing fused, dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z:
 *   lobe:      (r7, _) = philox_uniforms(seed, pixel, sample, 32 + d)  (streams 0-4, 8-11, 16-19, 24, 25 are taken);
 *              the hit is specular iff r7 < (double)p
 *   specular:  c = dot3(dir, n);  t = c + c;  nd = dir - n * t per component (not renormalised);  origin and source triangle as always
 *   diffuse:   unchanged: nd = rand_unit_vec(n, r1, r2), ct = dot3(nd, n)
 *   weights:   wS = 1.0f / p,  wD = 1.0f / (1.0f - p)  (IEEE f32 divisions), each used only when its lobe was taken
 *   unwind:    diffuse hit   rec_d = E_d + ((((brdf_d * rec_{d+1}) * ct_d) * (1/p_ref)) * wD)   (today's expression, 1/p_ref its 2 pi,
 *                            with one more scale; wD = 1.0f when p = 0)
 *              specular hit  rec_d = E_d + ((ks * rec_{d+1}) * wS)                               (per channel)
 *   E_d is the emission e_d of the plain estimator, D_d with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS:
 *              a specular hit draws no light sample and traces no shadow ray: L_d = 0
 *              Ew_d = e_d in full when d = 0 or hit d-1 was specular, else multiple importance sampling's e_d / (1 + u_b)
 *              D_d = Ew_d + L_d * wD (d = 0..3, per channel, L_d the light sample of multiple importance sampling),  D_4 = Ew_4
 *   so both strategies estimate the diffuse lobe's direct light given that lobe was chosen, and the mirror lobe carries everything
 *   it sees divided by p.  scans_executed counts what ran: no shadow scan for a specular hit. */

/* The context's specular table: n_tris * 4 f32 on the host for the scene last set (NULL clears the table); blocking, the array is
 * borrowed for the call; accepted by multi-device contexts (every device keeps the whole table, like the scene).  Every set_scene
 * clears the table.  During an accumulation it ends the accumulation as a set_scene does (the next step: SPHIP_E_STATE).
 * SPHIP_E_STATE without a scene; SPHIP_E_INVALID when a value is not finite, a ks < 0, p outside [0, 1] (the message names the first
 * such triangle; the table stays as it was) or the scene has 2^30 triangles or more (bit 30 of a triangle index marks a mirror bounce
 * in the kernels' path history). */
int sphip_set_specular(sphip_t* ctx, const float* spec);
/* The same from a device pointer, by the rules of sphip_set_scene_device: single-device contexts (SPHIP_E_STATE otherwise), ordered by
 * `stream` alone, and copied, so the caller may free d_spec once the stream has passed the call.  It does NOT validate the values:
 * a table that breaks the rules above gives undefined images (never out-of-bounds accesses). */
int sphip_set_specular_device(sphip_t* ctx, const void* d_spec, void* stream);

/* ---- smooth shading (SPHIP_FLAG_SMOOTH): per-vertex normals beside the scene, 9 f32 per triangle:
 * n0.xyz n1.xyz n2.xyz for v0 v1 v2.  Every hit of a path then shades with the normal interpolated at the hit point instead of the
 * triangle's stored one.  The normals need not be unit length (their lengths weigh the interpolation); a row of nine zeros leaves
 * that triangle flat.  The 12-float triangle and sphip_set_scene are unchanged.
 *
 * Valid for SPHIP_MODE_PT with the plain estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS, with variants 1, 8 (SPHIP_FLAG_ACCEL)
 * and 16 (both workgroup shapes), with SPHIP_FLAG_SPECULAR, SPHIP_FLAG_CAMERA_SAMPLES, progressive and adaptive accumulation,
 * denoising, sample chunks, primary-hit reuse, shards and multi-device contexts.  SPHIP_E_INVALID: with SPHIP_MODE_FLAT; with
 * SPHIP_FLAG_NEE without SPHIP_FLAG_MIS; with any other variant (2 and 15 are A/B scans: leaving them out halves the new kernels).
 * SPHIP_E_STATE: the flag without normals.  sphip_closest_hit_device ignores the flag.  Without the flag every render is bit for
 * bit what it is without normals; with the flag and a table of zeros too.
 *
 * The arithmetic, at hit d of a path on triangle i by the ray (o, dir); n is the triangle's stored normal turned against dir as
 * always, (n0, n1, n2) = the triangle's row; f32, every operation rounded on its own, nothing fused,
 * dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z:
 *   bary:    edge1, edge2, h, a, f = 1.0f / a, s, u = f * dot(s, h), q, v = f * dot(dir, q): exactly as the intersection test computes
 *            them for (o, dir, triangle i) (the reference's geom.h:200-212); recomputed for the winning triangle only, after the scan
 *   interp:  w = (1.0f - u) - v;  m = (n0 * w + n1 * u) + n2 * v per component;  l2 = dot3(m, m)
 *            sm = l2 > 0 and l2 finite.  !sm: ns = n, and the hit is in every respect what it is without the flag.
 *            sm:  ns = m / sqrtf(l2) per component (IEEE);  if dot3(ns, n) < 0: ns = -ns
 *   diffuse: nd = rand_unit_vec(ns, r1, r2);  ct = dot3(nd, ns);  sm and dot3(nd, n) < 0: the path ENDS after hit d
 *            (the hit keeps E_d; rec_{d+1} = 0; nothing more is scanned or counted)
 *   mirror:  c = dot3(dir, ns);  t = c + c;  nd = dir - ns * t;  sm and (!(c < 0) or dot3(nd, n) < 0): the path ends likewise
 *   light:   cos_x = dot3(wd, ns);  additionally, when sm, L_d = 0 without a shadow ray when !(dot3(wd, n) > 0)
 * Emitters keep their stored normal in cos_y, u_b and the light table (area densities are geometric).  Origins, source-triangle
 * skipping, the draw streams, wS, wD, Ew, D_d and the unwind expressions are unchanged; ct is simply the new value.  Both strategies
 * of multiple importance sampling integrate over the same set {w . ns > 0, w . n > 0}, so the plain estimator and NEE | MIS keep one
 * expectation.
 *
 * G-buffer: with the flag and normals set, sphip_gbuffer_device and sphip_accum_gbuffer store ns of the primary ray (the same
 * device function) where they store n otherwise; dist, albedo and mat are unchanged, and so is the filter.
 * sphip_selftest_device what 7: in f32[24 n] (pos dir v0 v1 v2 n0 n1 n2), out f32[6 n] (u, v, ns.xyz, sm as 0/1), the stored normal
 * taken as the reference's flat_normal of the vertices: the device function the kernels call. */

/* The context's vertex normals: n_tris * 9 f32 on the host for the scene last set (NULL clears them); blocking, the array is
 * borrowed for the call; accepted by multi-device contexts (every device keeps the whole table, like the scene).  Every set_scene
 * clears them.  During an accumulation it ends the accumulation as a set_scene does (the next step: SPHIP_E_STATE).
 * SPHIP_E_STATE without a scene; SPHIP_E_INVALID when a value is not finite (the message names the first such triangle; the table
 * stays as it was). */
int sphip_set_vertex_normals(sphip_t* ctx, const float* vn);
/* The same from a device pointer, by the rules of sphip_set_scene_device: single-device contexts (SPHIP_E_STATE otherwise), ordered by
 * `stream` alone, and copied, so the caller may free d_vn once the stream has passed the call.  It does NOT validate the values:
 * non-finite normals give undefined images (never out-of-bounds accesses: the table is indexed by triangle alone). */
int sphip_set_vertex_normals_device(sphip_t* ctx, const void* d_vn, void* stream);

/* ---- transparency (SPHIP_FLAG_DIELECTRIC): a per-triangle dielectric table beside the scene, 4 f32 per
 * triangle: kt.r, kt.g, kt.b, ior.  ior = 0 leaves the triangle what it is.  ior >= 1 makes it a smooth interface between vacuum, on
 * the side its stored normal points to, and a dielectric of index ior behind it: its diffuse reflectance and its row of the specular
 * table are ignored, its emittance still counts in E_d as always, and kt tints what is transmitted through it.  Every interface is
 * decided locally from the stored normal: there is no medium stack, and a ray that leaks through a mesh edge is simply in vacuum at
 * the next interface it meets from the normal's side.  The 6-float material and sphip_set_scene are unchanged.
 *
 * Valid for SPHIP_MODE_PT with the plain estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS, with variants 1, 8 (SPHIP_FLAG_ACCEL)
 * and 16 (both workgroup shapes), with or without SPHIP_FLAG_SPECULAR and SPHIP_FLAG_SMOOTH, with SPHIP_FLAG_CAMERA_SAMPLES,
 * progressive and adaptive accumulation, denoising (the G-buffer is unchanged), sample chunks, primary-hit reuse, shards and
 * multi-device contexts.  SPHIP_E_INVALID: with SPHIP_MODE_FLAT; with SPHIP_FLAG_NEE without SPHIP_FLAG_MIS; with any other variant
 * (2 and 15 are A/B scans, as for smooth shading).  SPHIP_E_STATE: the flag without a table.  Hit queries ignore the flag.  Without
 * the flag every render is bit for bit what it is without a table; with the flag and a table of zeros too.
 *
 * The arithmetic, at hit d of the path of (seed, global pixel, global sample) on triangle i with ior > 0 by the ray (o, dir); n is the
 * stored normal turned against dir as always, ns the shading normal (n, or shade_normal's under smooth shading),
 * entering = !(dot3(n_stored, dir) > 0); f32, every operation rounded on its own, nothing fused,
 * dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z, IEEE / and sqrtf:
 *   eta = entering ? 1.0f / ior : ior
 *   c   = dot3(dir, ns);  ci = -c
 *   k   = 1.0f - (eta * eta) * (1.0f - ci * ci);        tir = !(k > 0)
 *   ct  = sqrtf(k);  a = eta * ci;  b = eta * ct
 *   rs  = (a - ct) / (a + ct);  rp = (ci - b) / (ci + b);  Fr = 0.5f * (rs * rs + rp * rp)
 *   lobe:     (r7, _) = philox_uniforms(seed, pixel, sample, 32 + d)   (the specular lobe's stream: that lobe is not drawn on such a triangle)
 *             transmit iff !tir and (double)Fr <= r7   (a NaN Fr reflects);  otherwise reflect
 *   reflect:  nd = dir - ns * (c + c)   (the mirror's direction)      rec_d = E_d + rec_{d+1}
 *   transmit: nd = dir * eta + ns * (a - ct)   (per component)         rec_d = E_d + kt * rec_{d+1}   (per channel)
 * The origin x = o + dir * dist and source-triangle skipping are as always; nd is not renormalised.  Fresnel's probability and weight
 * cancel, so neither lobe carries a division.  There is no eta^2 radiance scale: camera paths start and end in vacuum.
 * Under smooth shading, when the hit is smooth (sm): the path ENDS after the hit when !(c < 0); a reflection ends it when
 * dot3(nd, n) < 0 (the mirror's rule); a transmission ends it when !(dot3(nd, n) < 0).
 * With SPHIP_FLAG_NEE | SPHIP_FLAG_MIS a hit on such a triangle is a specular hit in every respect: it draws no light sample and traces
 * no shadow ray, and the hit after it counts its emission in full (Ew_{d+1} = e_{d+1}).  Shadow rays treat glass as an occluder, so
 * light through glass is found by the BSDF strategy alone, with full weight: both estimators keep one expectation.  scans_executed
 * counts what ran.
 *
 * sphip_selftest_device what 8: in f32[8 n] (dir.xyz ns.xyz ior entering as 0/1), out f32[6 n] (Fr, tir as 0/1, nt.xyz, c), nt the
 * transmitted direction: the device function the kernels call (Fr and nt mean nothing when tir). */

/* The context's dielectric table: n_tris * 4 f32 on the host for the scene last set (NULL clears the table); blocking, the array is
 * borrowed for the call; accepted by multi-device contexts (every device keeps the whole table, like the scene).  Every set_scene
 * clears the table.  During an accumulation it ends the accumulation as a set_scene does (the next step: SPHIP_E_STATE).
 * SPHIP_E_STATE without a scene; SPHIP_E_INVALID when a value is not finite, a kt < 0, ior neither 0 nor >= 1 (the message names the
 * first such triangle; the table stays as it was) or the scene has 2^29 triangles or more (bit 29 of a triangle index marks a
 * transmitted bounce in the kernels' path history, beside bit 30 for every specular bounce). */
int sphip_set_dielectric(sphip_t* ctx, const float* glass);
/* The same from a device pointer, by the rules of sphip_set_specular_device: single-device contexts (SPHIP_E_STATE otherwise), ordered
 * by `stream` alone, and copied.  It does NOT validate the values: a table that breaks the rules above gives undefined images (never
 * out-of-bounds accesses: the table is indexed by triangle alone). */
int sphip_set_dielectric_device(sphip_t* ctx, const void* d_glass, void* stream);

/* ---- environment lighting: an octahedral radiance map beside the scene, n x n RGB texels (f32, row-major,
 * texel (i, j) at texels[(j * n + i) * 3], i along a, j along b) over the square (a, b) in [-1, 1]^2 with +y at the centre and -y at the
 * four corners, and the tables that importance-sample it.  SPHIP_FLAG_ENVIRONMENT lights SPHIP_MODE_PT renders with it: with the plain
 * estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS; variants 1, 8 (SPHIP_FLAG_ACCEL) and 16 in both workgroup shapes; with
 * SPHIP_FLAG_SPECULAR, _SMOOTH, _DIELECTRIC and _CAMERA_SAMPLES on or off; progressive and adaptive accumulation and denoising (the
 * G-buffer is unchanged and miss pixels pass through the filter: the background stays sharp), sample chunks, primary-hit reuse, shards
 * and multi-device contexts.  SPHIP_E_INVALID with SPHIP_MODE_FLAT, with SPHIP_FLAG_NEE without SPHIP_FLAG_MIS and with any other variant;
 * SPHIP_E_STATE for the flag without a map; hit queries ignore the flag.  Without the flag every render is bit for bit what it is without
 * a map, images and scans_executed, and with the flag and an all-zero map too.
 *
 * The arithmetic.  f32 unless marked double, every operation rounded on its own, nothing fused, dot3 as above, sgn(t) = t < 0 ? -1 : 1.
 *
 * env_lookup(d) -> (i, j, r3), for any non-zero d (the mapping does not depend on the scale of d: mirror and refracted directions are not
 * renormalised):
 *   s = (|d.x| + |d.y|) + |d.z|;  no texel when !(s > 0) or s is not finite
 *   p = d / s per component
 *   (a, b) = (p.x, p.z) when p.y >= 0, otherwise ((1 - |p.z|) sgn(p.x), (1 - |p.x|) sgn(p.z))
 *   i = clamp((int)((a * 0.5f + 0.5f) * (float)n), 0, n - 1);  j likewise from b
 *   l2 = dot3(p, p);  r3 = sqrtf(l2) * l2                       (da db = r3 d omega, on the folded half too: the fold is an isometry)
 *
 * The importance tables, in double, built by the library's own kernels behind both setters and equal to numpy's sequential cumsum:
 *   (a_c, b_c) = (-1 + (2 i + 1) / n, -1 + (2 j + 1) / n);  y_c = (1 - |a_c|) - |b_c|
 *   (x_c, z_c) = (a_c, b_c) when y_c >= 0, otherwise ((1 - |b_c|) sgn(a_c), (1 - |a_c|) sgn(b_c));  l2c = (x_c x_c + y_c y_c) + z_c z_c
 *   wt[j n + i]  = (((double)R + G) + B) / (sqrt(l2c) * l2c)
 *   rc[j][i]     = rc[j][i - 1] + wt[j n + i]   (one thread per row, in that order);  marg[j] = marg[j - 1] + rc[j][n - 1]   (one thread)
 *   T = marg[n - 1];  Phi = T * (4.0 / ((double)n * n))
 * and, with the scene (rebuilt on first use after the map or the scene changes), for the light table's environment entry:
 *   R2    = 0.25 * ((dx dx + dy dy) + dz dz), dx dy dz the extents of the bounding box of the scene's vertices, in double
 *   w_env = (0.5 * R2) * Phi   (the power through the scene's bounding disc, in the units A * Esum of the light table)
 *   W     = W_triangles + w_env;  when !(w_env > 0) (a black map: T = 0; a scene whose box is a point: R2 = 0) there is no entry: w_env = 0, W = W_triangles, tpdf = 0
 *   tpdf[t] = (float)(((w_env / W) * (wt[t] / T)) * ((double)n * n / 4.0))   (selection probability x density per unit (a, b) area)
 *
 * env_sample(r8, r9, r3, r4) -> (i, j, wd, r3), four uniforms in [0, 1) as doubles:
 *   j = the first row with marg[j] > r8 * T, the last if none;  i = the first column with rc[j][i] > r9 * rc[j][n - 1], the last if none
 *   a = ((float)i + (float)r3) * (2.0f / (float)n) - 1.0f;  b likewise from j, r4
 *   y = (1 - |a|) - |b|;  (x, z) = (a, b) when y >= 0, otherwise ((1 - |b|) sgn(a), (1 - |a|) sgn(b))
 *   g = (x, y, z);  l2 = dot3(g, g);  l = sqrtf(l2);  wd = g / l;  r3 = l * l2
 * The sample keeps the texel it was drawn from; env_lookup(wd) names the same texel except for a measured share of draws on texel
 * edges.
 *
 * The flagged light table.  With the flag the context keeps a second light table beside the unflagged one: the triangle entries as in
 * "next-event estimation", plus, when w_env > 0, one last entry for the map, of weight w_env; the running sum ends in W = W_triangles + w_env
 * and every ipdf is (float)(W / Esum) under that W.  A map without an entry (all zero) leaves W, ipdf and every bit as without the flag.
 *
 * Balance ratio against the BSDF density q = 1 / (pi^2 sxz), as in mis_u:  u_env(sxz, r3, t) = ((kPiSq * sxz) * r3) * tpdf[t], 0 where
 * that is NaN.
 *
 * Light sample at hit d, d = 0..3 (NEE|MIS).  r5 selects the table entry as for triangles.  When it is the map's entry:
 *   (r8, r9) = philox_uniforms(seed, pixel, sample, 40 + d);  (i, j, wd, r3) = env_sample(r8, r9, r3, r4), (r3, r4) of stream 8 + d
 *   t = j n + i: the sample keeps its texel for Le and tpdf, there is no second lookup
 *   cos_x = dot3(wd, ns); no sample when !(cos_x > 0); under smooth shading smooth_light_ok applies
 *   the shadow ray (x, wd) skips src with tmax = 1e12f and is occluded iff anything is hit; one scan in scans_executed
 *   L_d = (reflectance_src * (1/pi)) * (Le_t * ((kTwoPi * cos_x) / (1 + u_env(sxz(wd), r3, t)))), then the wD scale as for triangle lights
 * It never exceeds 2 reflectance Le.  A specular or glass hit draws no light sample.
 *
 * Miss of the ray of depth d, d = 0..4:  (i, j, r3) = env_lookup(dir), t = j n + i, Le = texels[t] (0 without a texel).
 *   plain estimator:  E_miss = Le
 *   NEE|MIS:          E_miss = Le when d = 0, when hit d - 1 was specular or transmitted, or when !(tpdf[t] > 0);
 *                     otherwise Le / (1 + u_env(sqrtf(dir.x dir.x + dir.z dir.z), r3, t)) per channel
 * The unwind starts from rec = E_miss at a miss, where it starts from 0 without the flag; a path that ends for any other reason (the
 * fifth hit, the smooth and glass ending rules) starts from 0.  The primary miss makes the map the background, and
 * SPHIP_FLAG_CAMERA_SAMPLES antialiases it like anything else. */

/* The context's environment map: n * n * 3 f32 on the host (NULL clears the map); blocking, the array is borrowed for the call; accepted
 * by multi-device contexts (every device keeps the map and its tables).  Unlike the per-triangle tables the map is NOT cleared by
 * sphip_set_scene and needs no scene (the scene-dependent part, w_env, W and tpdf, is rebuilt with the flagged light table on the first
 * flagged render after either changes).  During an accumulation it ends the accumulation as sphip_set_specular does.  SPHIP_E_INVALID for
 * n == 0, for n > 2048, or for a value that is negative or not finite (the message names the first such texel; the map stays as it was). */
int sphip_set_environment(sphip_t* ctx, const float* texels, uint32_t n);
/* The same from a device pointer, by the rules of sphip_set_specular_device: single-device contexts (SPHIP_E_STATE otherwise), ordered
 * by `stream` alone (the tables are built on it), and copied.  It does NOT validate the values: a map that breaks the rules above gives
 * undefined tables (never out-of-bounds accesses: n is checked, and every table index is bounded by n). */
int sphip_set_environment_device(sphip_t* ctx, const void* d_texels, uint32_t n, void* stream);
/* TEST-ONLY: copies out the tables above for the context's map and scene (SPHIP_E_STATE without either).  *n_out: the map's n; call with
 * the other outputs NULL first to size them (each may be NULL on its own): out_wt f64[n n], out_rc f64[n n], out_marg f64[n],
 * out_tpdf f32[n n], out_T_wenv_W f64[3] = T, w_env, W.  Blocking; host pointers; on a multi-device context the first device's.
 * This call and sphip_selftest_device what 9 and 10 read the tables on the context's own stream: after sphip_set_environment_device the
 * caller synchronises the stream it gave before calling them (nothing else orders the two streams). */
int sphip_selftest_env_dump(sphip_t* ctx, uint32_t* n_out, double* out_wt, double* out_rc, double* out_marg, float* out_tpdf, double* out_T_wenv_W);

/* ---- glossy reflection (SPHIP_FLAG_GLOSSY): a per-triangle roughness table beside the scene, 1 f32 per triangle:
 * the GGX alpha of the triangle's mirror lobe (the lobe of its row of the specular table).  alpha = 0 leaves the lobe the perfect mirror,
 * bit for bit; alpha > 0 reflects about a microfacet normal drawn from the GGX distribution of visible normals (Heitz 2018) and weights
 * the sample by the separable Smith term of the outgoing direction, so the weight of a glossy hit is ks g / p <= ks / p: bounded as a
 * mirror's is.  On a dielectric triangle (ior > 0) the row is ignored: rough glass is out of scope.
 *
 * Valid for SPHIP_MODE_PT together with SPHIP_FLAG_SPECULAR, with the plain estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS, with
 * variants 1, 8 (SPHIP_FLAG_ACCEL) and 16 in both workgroup shapes, with SPHIP_FLAG_SMOOTH, SPHIP_FLAG_DIELECTRIC, SPHIP_FLAG_ENVIRONMENT
 * and SPHIP_FLAG_CAMERA_SAMPLES on or off, with progressive and adaptive accumulation and denoising (the G-buffer is unchanged), sample
 * chunks, primary-hit reuse, shards and multi-device contexts.  SPHIP_E_INVALID: with SPHIP_MODE_FLAT; with SPHIP_FLAG_NEE alone; with
 * variants 2, 15 or a retired one; without SPHIP_FLAG_SPECULAR.  SPHIP_E_STATE: the flag without a roughness table.  Hit queries ignore
 * the flag.  Without the flag every render is bit for bit what it is without a table; with the flag and a table of zeros too.
 *
 * The estimator, at hit d of the path of (seed, global pixel, global sample) on triangle i, when the lobe drawn is specular (the lobe
 * rule of "specular reflection", unchanged), glass[i].w is not positive and al = rough[i] > 0.  dir: the ray; ns: the shading normal
 * turned against dir, the stored one or smooth shading's; c = dot3(dir, ns).  f32 unless marked, every operation rounded on its own,
 * nothing fused; dot3 as above, cross3(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x):
 *   draws:   (u1, u2) = philox_uniforms(seed, pixel, sample, 48 + d)   (streams 0-4, 8-11, 16-19, 24, 25, 32-36, 40-43 are taken)
 *   frame:   sg = ns.z < 0 ? -1 : 1;  a = -1.0f / (sg + ns.z);  b = (ns.x * ns.y) * a
 *            t  = (1.0f + (sg * (ns.x * ns.x)) * a,  sg * b,  (-sg) * ns.x)
 *            bt = (b,  sg + (ns.y * ns.y) * a,  -ns.y)
 *   view:    v  = (-dot3(dir, t), -dot3(dir, bt), -c)
 *   stretch: h  = (al v.x, al v.y, v.z);  vh = h / sqrtf(dot3(h, h)) per component
 *   basis:   l2 = vh.x * vh.x + vh.y * vh.y;  T1 = l2 > 0 ? (-vh.y / sqrtf(l2), vh.x / sqrtf(l2), 0) : (1, 0, 0);  T2 = cross3(vh, T1)
 *   disk:    r = (float)sqrt(u1) (a double sqrt);  phi = (float)((u2 * pi) * 2.0) (double, as the lens);  (sn, cs) = sincos_glibc(phi)
 *            p1 = r * cs;  p2 = r * sn;  s = 0.5f * (1.0f + vh.z);  q = 1.0f - p1 * p1;  q = q > 0 ? q : 0
 *            p2 = (1.0f - s) * sqrtf(q) + s * p2
 *            z2 = (1.0f - p1 * p1) - p2 * p2;  z = sqrtf(z2 > 0 ? z2 : 0)
 *            nh = (T1 * p1 + T2 * p2) + vh * z
 *   normal:  ne = (al nh.x, al nh.y, nh.z > 0 ? nh.z : 0);  ml = ne / sqrtf(dot3(ne, ne));  m = (t * ml.x + bt * ml.y) + ns * ml.z
 *   bounce:  nd = dir - m * (cm + cm), cm = dot3(dir, m)   (not renormalised, like the mirror's)
 *   weight:  cl = dot3(nd, ns);  ok = cl > 0;  g = (cl + cl) / (cl + sqrtf(al * al + (1.0f - al * al) * (cl * cl)));  g = g > 1 ? 1 : g
 * cl stands for the cosine although nd has dir's length, which is unit up to rounding after mirrors and refraction; the last select
 * keeps g <= 1, and so the weight ks g / p <= ks / p, when that rounding puts cl above 1.
 *   ending:  the path ends after the hit when !ok: the hit keeps E_d, rec_{d+1} = 0 (g_d counts as 0), nothing more is scanned or
 *            counted.  On a smooth hit the mirror's two rules apply as well: sm && (!(c < 0) || dot3(nd, n) < 0)
 *   unwind:  rec_d = E_d + (((ks * rec_{d+1}) * wS) * g_d) per channel; at al = 0 (and after !ok) the mirror's expression with its bits
 * With SPHIP_FLAG_NEE | SPHIP_FLAG_MIS a glossy hit is a specular hit in every respect: it draws no light sample and traces no shadow
 * ray, and the next hit or miss counts its emission in full, so both estimators keep one expectation by the mirror's argument. */

/* The context's roughness table: n_tris f32 on the host for the scene last set (NULL clears the table), by the rules of
 * sphip_set_specular: blocking; accepted by multi-device contexts; cleared by every set_scene; during an accumulation it ends the
 * accumulation as a set_scene does.  SPHIP_E_STATE without a scene; SPHIP_E_INVALID when a value is not finite or lies outside [0, 1]
 * (the message names the first such triangle; the table stays as it was). */
int sphip_set_roughness(sphip_t* ctx, const float* alpha);
/* The same from a device pointer, by the rules of sphip_set_specular_device: single-device contexts (SPHIP_E_STATE otherwise), ordered by
 * `stream` alone, and copied.  It does NOT validate the values: a table that breaks the rules above gives undefined images (never
 * out-of-bounds accesses). */
int sphip_set_roughness_device(sphip_t* ctx, const void* d_alpha, void* stream);

/* ---- textures (SPHIP_FLAG_TEXTURE): a per-triangle UV table beside the scene, 6 f32 per triangle: s0 t0 s1 t1 s2 t2
 * for v0 v1 v2, and one atlas on the context, tw x th RGB texels, f32, row-major: texel (i, j) at texels[(j * tw + i) * 3], row 0 at
 * t = 0.  With the flag the diffuse reflectance of a hit on a textured triangle is albedo = rho * c per channel: rho the material's
 * reflectance, c the bilinear sample of the atlas at the hit's interpolated UV, with repeat addressing.  albedo replaces rho in exactly
 * two places: the unwind's brdf_d = albedo * (1 / pi), and the reflectance of the hit in its light sample L_d (a triangle light's and
 * the map's).  Nothing else reads it: ks, kt, the emittance, the light table, the G-buffer (its albedo and mat stay the material's),
 * the flat pass and hit queries are unchanged, and so is scans_executed: a texture traces nothing.  A row of the UV table whose six
 * values all compare equal to 0.0f leaves its triangle untextured (as nine zero normals leave a triangle flat).
 *
 * Valid for SPHIP_MODE_PT with the plain estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS, with variants 1, 8 (SPHIP_FLAG_ACCEL) and 16
 * in both workgroup shapes, with SPHIP_FLAG_SPECULAR, SPHIP_FLAG_GLOSSY, SPHIP_FLAG_DIELECTRIC, SPHIP_FLAG_ENVIRONMENT, SPHIP_FLAG_SMOOTH
 * and SPHIP_FLAG_CAMERA_SAMPLES on or off, with progressive and adaptive accumulation and denoising, sample chunks, primary-hit reuse,
 * shards and multi-device contexts.  SPHIP_E_INVALID: with SPHIP_MODE_FLAT; with SPHIP_FLAG_NEE alone; with variants 2, 15 or a retired
 * one.  SPHIP_E_STATE: the flag without a UV table (checked first), or without an atlas.  Hit queries ignore the flag.  Without the
 * flag every render is bit for bit what it is without a table; with the flag and a table of zeros too.
 *
 * The arithmetic at a hit on triangle i by ray (o, dir).  f32, every operation rounded on its own, nothing fused:
 *   bary:    u, v exactly as smooth shading computes them (geom.h:200-212), for the winning triangle, after the scan
 *   interp:  w = (1.0f - u) - v;  s = (s0 * w + s1 * u) + s2 * v;  t likewise
 *            textured iff the row is not all zero and s, t are finite; otherwise albedo = rho: the hit is in every respect what it is
 *            without the flag
 *   wrap:    fs = s - floorf(s);  fs = fs < 1.0f ? fs : 0.0f;  ft likewise                       (repeat addressing)
 *   texel:   x = fs * (float)tw - 0.5f;  x0 = floorf(x);  fx = x - x0;  i0 = (int)x0;  i0 = i0 < 0 ? i0 + tw : i0;
 *            i1 = i0 + 1 == tw ? 0 : i0 + 1;  y, y0, fy, j0, j1 likewise with th
 *   lerp:    top = t00 + (t10 - t00) * fx;  bot = t01 + (t11 - t01) * fx;  c = top + (bot - top) * fy   (per channel; tIJ = texel (iI, jJ))
 *   albedo:  rho * c per channel
 * Where the four texels of a footprint are equal, c is that texel bit for bit: the lerp form is chosen for that. */

/* The context's atlas: tw x th x 3 f32 on the host (NULL clears it), by the rules of sphip_set_environment: blocking; accepted by
 * multi-device contexts (every device keeps the atlas); kept across set_scene and needs no scene; during an accumulation it ends the
 * accumulation as a set_scene does.  SPHIP_E_INVALID when tw or th is 0 or above 4096, or a value is negative or not finite (the message
 * names the first such texel; the atlas stays as it was). */
int sphip_set_texture(sphip_t* ctx, const float* texels, uint32_t tw, uint32_t th);
/* The same from a device pointer, by the rules of sphip_set_environment_device: single-device contexts (SPHIP_E_STATE otherwise),
 * ordered by `stream` alone, and copied.  It does NOT validate the values: texels that break the rules above give undefined images
 * (never out-of-bounds accesses). */
int sphip_set_texture_device(sphip_t* ctx, const void* d_texels, uint32_t tw, uint32_t th, void* stream);
/* The context's UV table: n_tris * 6 f32 on the host for the scene last set (NULL clears the table), by the rules of
 * sphip_set_specular: blocking; accepted by multi-device contexts; cleared by every set_scene; during an accumulation it ends the
 * accumulation as a set_scene does.  SPHIP_E_STATE without a scene; SPHIP_E_INVALID when a value is not finite (the message names the
 * first such triangle; the table stays as it was). */
int sphip_set_uv(sphip_t* ctx, const float* uv);
/* The same from a device pointer, by the rules of sphip_set_specular_device.  It does NOT validate the values: a hit whose
 * interpolated UV is not finite is untextured (never out-of-bounds accesses). */
int sphip_set_uv_device(sphip_t* ctx, const void* d_uv, void* stream);

/* ---- normal mapping (SPHIP_FLAG_NORMAL_MAP): one normal map on the context, nw x nh RGB texels, f32, laid out like the
 * atlas: texel (i, j) at texels[(j * nw + i) * 3], row 0 at t = 0.  A texel holds a tangent-space vector (x, y, z) as signed floats (NOT
 * the 0..1 encoding of image files: decoding is the host's job), x along increasing s, y along increasing t, z along the surface normal.
 * The map is addressed by the scene's UV table (sphip_set_uv) and sampled as the atlas is, with the wrap, texel and lerp steps of
 * "textures" unchanged.  With the flag every hit of a path replaces its shading normal ns by the map's normal in the hit's tangent frame,
 * and is from there on a smooth hit (sm = true) in every rule of "smooth shading": the diffuse, mirror, glossy and glass bounces, the
 * light sample's cosine and its guard against the stored normal, and the ending rules all read ns and sm as they do under
 * SPHIP_FLAG_SMOOTH.  Emitters keep their stored normal; scans_executed is unchanged: a map traces nothing.
 *
 * Valid for SPHIP_MODE_PT with the plain estimator and with SPHIP_FLAG_NEE | SPHIP_FLAG_MIS, with variants 1, 8 (SPHIP_FLAG_ACCEL) and 16
 * in both workgroup shapes, with every material and lighting flag (SPHIP_FLAG_SPECULAR, SPHIP_FLAG_GLOSSY, SPHIP_FLAG_DIELECTRIC,
 * SPHIP_FLAG_ENVIRONMENT, SPHIP_FLAG_SMOOTH, SPHIP_FLAG_TEXTURE) and SPHIP_FLAG_CAMERA_SAMPLES on or off, with progressive and adaptive
 * accumulation and denoising, sample chunks, primary-hit reuse, shards and multi-device contexts.  SPHIP_E_INVALID: with SPHIP_MODE_FLAT;
 * with SPHIP_FLAG_NEE alone; with variants 2, 15 or a retired one.  SPHIP_E_STATE: the flag without a UV table (checked first), or
 * without a normal map.  Hit queries ignore the flag.
 *
 * The step runs at a hit on triangle i by ray (o, dir), after smooth shading's.  n: the stored normal turned against dir; ns, sm: what
 * smooth shading left (n, false on a flat triangle or without SPHIP_FLAG_SMOOTH); s0 t0 s1 t1 s2 t2: the triangle's UV row.  f32, every
 * operation rounded on its own, nothing fused; dot3 and cross3 as above:
 *   bary:    u, v exactly as smooth shading and textures compute them;  w = (1.0f - u) - v
 *            s = (s0 * w + s1 * u) + s2 * v;  t likewise                                         (textures' interp)
 *   texel:   m = the bilinear sample of the map at (s, t)                                        (wrap, texel, lerp of "textures")
 *   frame:   e1 = v1 - v0;  e2 = v2 - v0
 *            ds1 = s1 - s0;  ds2 = s2 - s0;  dt1 = t1 - t0;  dt2 = t2 - t0
 *            det = ds1 * dt2 - ds2 * dt1;  sg = det < 0 ? -1.0f : 1.0f
 *            T = (e1 * dt2 - e2 * dt1) * sg;  B = (e2 * ds1 - e1 * ds2) * sg                     (per component)
 *            Tp = T - ns * dot3(ns, T);  lt = dot3(Tp, Tp);  Tn = Tp / sqrtf(lt)                 (per component, IEEE)
 *            C = cross3(ns, Tn);  h = dot3(C, B) < 0 ? -1.0f : 1.0f;  Bn = C * h
 *   normal:  p = (Tn * m.x + Bn * m.y) + ns * m.z;  lp = dot3(p, p);  np = p / sqrtf(lp)
 * The hit is perturbed (ns = np, sm = true) iff all of these hold: the UV row is not all zero and s, t are finite (textures' rule);
 * det > 0 || det < 0;  lt > 0 and finite;  not (m.x == 0 && m.y == 0);  m.z > 0;  lp > 0 and finite;  dot3(np, n) > 0;
 * dot3(dir, np) < 0.  Otherwise ns and sm stay what smooth shading left, and the hit is in every respect what it is without the flag.
 *   - A map of (0, 0, 1) everywhere, or a row of zero UVs, is "no flag" bit for bit.
 *   - The last two guards fall back to the unmapped normal; they do not end the path, so a steep texel seen at a grazing angle gives no
 *     black fringe.
 *   - On a back-face hit ns already points to the ray's side: the bump keeps its x, y and inverts its depth.
 * Both estimators keep one expectation by smooth shading's argument: ns is a function of the hit and the incoming ray, identical in
 * the plain and the NEE|MIS path.
 * G-buffer: with the flag sphip_gbuffer_device and sphip_accum_gbuffer store the perturbed ns of the primary ray where they store ns or n
 * without it; dist, albedo and mat are unchanged.
 * sphip_selftest_device what 13 (nmap_normal): in f32[30 n] = pos dir v0 v1 v2 n0 n1 n2 uv0 uv1 uv2, out f32[6 n] = s, t, ns.xyz,
 * perturbed (0/1), against the context's map (SPHIP_E_STATE without one); the stored normal is the flat normal of the vertices, as in
 * what 7. */

/* The context's normal map: nw x nh x 3 f32 on the host (NULL clears it), by the rules of sphip_set_texture: blocking; accepted by
 * multi-device contexts (every device keeps the map); kept across set_scene and needs no scene; during an accumulation it ends the
 * accumulation as a set_scene does.  SPHIP_E_INVALID when nw or nh is 0 or above 4096, or a value is not finite (negative values are
 * legal; the message names the first such texel; the map stays as it was). */
int sphip_set_normal_map(sphip_t* ctx, const float* texels, uint32_t nw, uint32_t nh);
/* The same from a device pointer, by the rules of sphip_set_texture_device: single-device contexts (SPHIP_E_STATE otherwise), ordered by
 * `stream` alone, and copied.  It does NOT validate the values: texels that break the rule above give undefined images (never
 * out-of-bounds accesses). */
int sphip_set_normal_map_device(sphip_t* ctx, const void* d_texels, uint32_t nw, uint32_t nh, void* stream);

/* Blocks until the last render on this context has finished, then reports its figures. */
int sphip_get_stats(sphip_t* ctx, sphip_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SPATH_HIP_H */
