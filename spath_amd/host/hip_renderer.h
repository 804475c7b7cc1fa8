// hip_renderer -- the MI355X backend as a peer of cpu_renderer / cl_renderer / vk_renderer.
// Same shape as the reference's per-backend headers (src/cpu_renderer.h:23-25): one factory.
#pragma once

#include "spath_iface.h"
#include "spath_hip.h"

#include <stdint.h>

namespace hip_renderer {
	// Returns a new renderer owned by the caller (the reference wraps it in std::unique_ptr,
	// src/main.cpp:242-244).  Throws std::runtime_error when no usable HIP device exists, like the
	// reference's GPU peers do from their constructors (src/cl_renderer.cpp:155-187).
	// One GPU: device 0 (or the devices listed in the environment variable SPATH_HIP_DEVICES, e.g. "0,1,2,3").
	extern scene::renderer* get(const int w, const int h);
	// Opt-in: several GPUs of the node behind one renderer -- pixel-row tiles dealt round-robin, one gather to the first device,
	// same image bit for bit as on one GPU.  An explicit device list (a device may be listed more than once), or every visible GPU.
	extern scene::renderer* get_on(const int w, const int h, const int* device_ids, const int n_devices);
	extern scene::renderer* get_all_devices(const int w, const int h);
	extern int device_count(scene::renderer* r);

	// Optional knobs of this backend (not part of the reference interface): the RNG seed of the next
	// frames and the C-ABI flags word (kernel variant, primary-hit reuse; see include/spath_hip.h).
	extern void set_seed(scene::renderer* r, unsigned long long seed);
	extern void set_flags(scene::renderer* r, int flags);
	// next-event estimation on or off (SPHIP_FLAG_NEE in the flags word; include/spath_hip.h): light sampling with shadow rays,
	// a less noisy estimate of the same image
	extern void set_nee(scene::renderer* r, bool on);
	// next-event estimation with multiple importance sampling (SPHIP_FLAG_NEE | SPHIP_FLAG_MIS): on sets both flags, off clears
	// SPHIP_FLAG_MIS only (NEE stays as set_nee left it); the same image again, without NEE's fireflies
	extern void set_mis(scene::renderer* r, bool on);
	// per-sample camera rays (SPHIP_FLAG_CAMERA_SAMPLES; include/spath_hip.h "camera samples"): pixel antialiasing and, with a lens,
	// depth of field.  Honoured by render_own_viewport only: render() takes the caller's rays and renders exactly as without it.
	extern void set_camera_samples(scene::renderer* r, bool on);
	// the thin lens of camera samples (sphip_set_lens): aperture 0 = pinhole; throws std::runtime_error on values the library refuses.
	// The lens joins the key of a progressive accumulation on the camera path
	extern void set_lens(scene::renderer* r, float aperture, float focus_dist);
	// specular reflection (sphip_set_specular, SPHIP_FLAG_SPECULAR; include/spath_hip.h "specular reflection"): a table of n_tris rows
	// ks.r ks.g ks.b p (copied) beside the materials of the scenes rendered next; while one is set, path-traced frames mirror by it
	// (render_flat is unchanged).  NULL or n_tris = 0 removes it.  A table the library refuses makes the next frame throw
	// std::runtime_error, as does one whose size differs from the scene's.  Changing it begins a new progressive accumulation.
	extern void set_specular(scene::renderer* r, const float* spec, size_t n_tris);
	// smooth shading (sphip_set_vertex_normals, SPHIP_FLAG_SMOOTH; include/spath_hip.h "smooth shading"): n_tris rows n0.xyz n1.xyz
	// n2.xyz (copied) beside the triangles of the scenes rendered next; while they are set, path-traced frames shade by them
	// (render_flat is unchanged).  NULL or n_tris = 0 removes them.  Normals the library refuses make the next frame throw
	// std::runtime_error, as do ones whose size differs from the scene's.  Changing them begins a new progressive accumulation.
	extern void set_vertex_normals(scene::renderer* r, const float* vn, size_t n_tris);
	// transparency (sphip_set_dielectric, SPHIP_FLAG_DIELECTRIC; include/spath_hip.h "transparency"): a table of n_tris rows
	// kt.r kt.g kt.b ior (copied) beside the materials of the scenes rendered next; while one is set, path-traced frames refract by it
	// (render_flat is unchanged).  NULL or n_tris = 0 removes it.  A table the library refuses makes the next frame throw
	// std::runtime_error, as does one whose size differs from the scene's.  Changing it begins a new progressive accumulation.
	extern void set_dielectric(scene::renderer* r, const float* glass, size_t n_tris);
	// glossy reflection (sphip_set_roughness, SPHIP_FLAG_GLOSSY; include/spath_hip.h "glossy reflection"): n_tris GGX alphas (copied)
	// beside the specular table of the scenes rendered next; while they are set, path-traced frames roughen the mirror lobe by them
	// (render_flat is unchanged; the library refuses the frame without a specular table).  NULL or n_tris = 0 removes them.  A table the
	// library refuses makes the next frame throw std::runtime_error, as does one whose size differs from the scene's.  Changing it
	// begins a new progressive accumulation.
	extern void set_roughness(scene::renderer* r, const float* alpha, size_t n_tris);
	// textures (sphip_set_texture, sphip_set_uv, SPHIP_FLAG_TEXTURE; include/spath_hip.h "textures"): an atlas of tw x th x 3 floats and
	// a UV table of n_tris x 6 floats (both copied); while both are set, path-traced frames scale the diffuse reflectance of every hit
	// by the atlas at the hit's UV (render_flat is unchanged).  NULL or a zero size removes either.  An atlas or a table the library
	// refuses makes the next frame throw std::runtime_error, as does a table whose size differs from the scene's.  Changing either
	// begins a new progressive accumulation.
	extern void set_texture(scene::renderer* r, const float* texels, uint32_t tw, uint32_t th);
	extern void set_uv(scene::renderer* r, const float* uv, size_t n_tris);
	// normal mapping (sphip_set_normal_map, SPHIP_FLAG_NORMAL_MAP; include/spath_hip.h "normal mapping"): a map of nw x nh x 3 floats, signed
	// tangent-space vectors (copied), addressed by the UV table of set_uv; while a map and a UV table are both set, path-traced frames
	// shade every hit with the map's normal (render_flat is unchanged).  NULL or a zero size removes it.  A map the library refuses makes
	// the next frame throw std::runtime_error.  Changing it begins a new progressive accumulation.
	extern void set_normal_map(scene::renderer* r, const float* texels, uint32_t nw, uint32_t nh);
	// environment lighting (sphip_set_environment, SPHIP_FLAG_ENVIRONMENT; include/spath_hip.h "environment lighting"): an octahedral
	// radiance map of n x n x 3 floats (copied); while one is set, path-traced frames are lit by it and show it behind the scene
	// (render_flat is unchanged).  NULL or n = 0 removes it.  A map the library refuses makes the next frame throw std::runtime_error.
	// Changing it begins a new progressive accumulation.
	extern void set_environment(scene::renderer* r, const float* texels, uint32_t n);
	// Progressive rendering for a viewer whose view stands still (off by default: render() then behaves like the reference's).
	// When on, render() adds its n_samples to the samples of the previous calls while the viewport rays (compared bit for bit),
	// the scene, the seed and the flags are unchanged, and the bitmap is the image of all of them -- bit-identical to one
	// render of their sum; any change begins a new accumulation.  render_own_viewport does the same, keyed on the camera.
	// render_flat is not accumulated.  Switching the mode (on or off) also begins anew.
	extern void set_progressive(scene::renderer* r, bool on);
	// Adaptive sampling of the progressive mode (include/spath_hip.h: sphip_accum_begin_adaptive): converged pixels stop, each
	// keeping exactly the image of its own sample count.  t < 0 turns it off (the default).  Switching on or off, or changing the
	// rule, begins anew.
	extern void set_adaptive(scene::renderer* r, double t, double floor, unsigned min_samples);
	// Denoising of the progressive mode (include/spath_hip.h: sphip_accum_denoise): with p != NULL the bitmap of every progressive
	// step is the accumulation denoised with *p (copied), and the raw image stays reachable through raw_bitmap.  Without an
	// adaptive rule the accumulation is begun with one that never stops a pixel (min_samples = UINT32_MAX), so that the filter has
	// the variance; the raw image is bit-identical to a plain accumulation's.  NULL turns it off (the default).
	extern void set_denoise(scene::renderer* r, const sphip_denoise* p);
	// Temporal reprojection of the progressive mode (include/spath_hip.h: sphip_accum_reproject): with p != NULL (copied), a camera move
	// (set_delta_mov / set_delta_rot / set_delta_focal) between two render_own_viewport frames no longer begins a new accumulation: the
	// old view's accumulation is reprojected into the new view and blended with its samples, drawn under seed + the number of moves
	// reprojected so far.  Every other cause still begins anew: a scene, table or image change, a resize, the lens, the seed, the flags,
	// the adaptive rule, and render() (the caller's rays carry no camera).  With denoising on, the accumulation is plain and the filter
	// runs without the variance.  Refused (std::runtime_error with the library's message) while an adaptive rule is set, as set_adaptive
	// is while this is on.  NULL turns it off (the default).
	extern void set_reproject(scene::renderer* r, const sphip_reproject* p);
	// Display transform of the progressive mode (include/spath_hip.h: sphip_accum_display): with p != NULL (copied) the bitmap of every
	// progressive step goes through exposure, tone curve and encoding instead of the linear clamp; with m != NULL (copied) the exposure is
	// metered from each step's image, else it is p->exposure.  Composes with set_denoise (the filtered image is what is shown, and
	// metered; raw_bitmap stays the clamp-only raw image) and with set_reproject (the blended mean).  A post-process: switching it on, off
	// or changing it does not begin a new accumulation.  NULL turns it off (the default).  Like set_denoise it may be called before
	// set_progressive and is kept: it acts on the progressive path-traced frames only, and every other frame (render_flat, or render with
	// the progressive mode off) is the linear clamp as before.  (The Python HipRenderer fixes the progressive mode at construction and
	// therefore refuses set_display on a renderer that is not progressive.)
	extern void set_display(scene::renderer* r, const sphip_display* p, const sphip_metering* m);
	// the exposure the last progressive step was shown with (the metered one with metering on); 1 without a display transform
	extern float display_exposure(scene::renderer* r);
	// the raw (not denoised) image of the last progressive step with denoising on; NULL if r is not a hip renderer or there is none
	extern const scene::bitmap* raw_bitmap(scene::renderer* r);
	// per-pixel sample counts (w*h, image order) and active pixels of the current accumulation; false if r is not a hip renderer
	// or no accumulation is live
	extern bool accum_counts(scene::renderer* r, uint32_t* counts, unsigned long long* n_active);
	// get_viewport + render (or render_flat) with the viewport generated on the device from the renderer's own
	// camera (bit-identical rays, no 24 B/pixel upload).  Returns false if r is not a hip renderer.
	extern bool render_own_viewport(scene::renderer* r, const geom::triangle* tris, const scene::material* mats, const size_t n_tris,
	                                const size_t n_samples, scene::bitmap& out, const bool flat);
	// kernel milliseconds and closest-hit scans of the last frame (0 if r is not a hip renderer)
	extern bool last_stats(scene::renderer* r, double* kernel_ms, unsigned long long* scans);
}
