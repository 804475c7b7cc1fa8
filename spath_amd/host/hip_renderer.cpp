// The C++ adapter between the reference's plugin interface and the C ABI of libspath_hip.so.
//
// hip_r derives from basic_renderer exactly like the reference's pt_r / cl_r / vk_r do
// (src/cpu_renderer.cpp:186-202, src/cl_renderer.cpp:90-257), so the five camera virtuals come from
// the shared mix-in and only get_description / render_flat / render are implemented here.
// Compiles against the reference's own headers (-DSPATH_REFERENCE_HEADERS -I<spath>/src) or against
// the compatible declarations in spath_iface.h.
#include "hip_renderer.h"

#include "spath_hip.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

static_assert(sizeof(geom::triangle) == 48 && sizeof(geom::ray) == 24 && sizeof(scene::material) == 24 && sizeof(scene::RGBA) == 4,
              "the C ABI takes the reference's packed structs as plain float arrays");

// What a frame depends on beside the triangles and the materials: the per-triangle tables and the three context-level images, in the
// order in which they follow the scene to the library.  One rule for all: kept by its setter (hip_renderer::set_X), it joins the scene's
// key and goes to the library with every scene upload (sphip_set_scene clears the tables; the library keeps the images across scenes,
// but they travel like the tables so that one key covers everything); while everything that carries a flag is set, path-traced frames
// carry that flag.
enum part_id { P_ENV, P_SPEC, P_VNORM, P_GLASS, P_ROUGH, P_TEX, P_NMAP, P_UV, N_PARTS };
int set_env_image(sphip_t* c, const float* texels, uint32_t n, uint32_t) { return sphip_set_environment(c, texels, n); }
struct part_rule {
	const char* what;                                                // the call, as check() names it
	int flag;
	size_t floats;                                                   // per triangle; 0: an image of w x h x 3 floats
	const char* noun;                                                // of a table, for the size check
	int (*set_table)(sphip_t*, const float*);
	int (*set_image)(sphip_t*, const float*, uint32_t, uint32_t);
};
const part_rule part_rules[N_PARTS] = {
	{ "set_environment", SPHIP_FLAG_ENVIRONMENT, 0, 0, 0, set_env_image },
	{ "set_specular", SPHIP_FLAG_SPECULAR, 4, "specular table", sphip_set_specular, 0 },
	{ "set_vertex_normals", SPHIP_FLAG_SMOOTH, 9, "vertex normals", sphip_set_vertex_normals, 0 },
	{ "set_dielectric", SPHIP_FLAG_DIELECTRIC, 4, "dielectric table", sphip_set_dielectric, 0 },
	{ "set_roughness", SPHIP_FLAG_GLOSSY, 1, "roughness table", sphip_set_roughness, 0 },
	{ "set_texture", SPHIP_FLAG_TEXTURE, 0, 0, 0, sphip_set_texture },
	{ "set_normal_map", SPHIP_FLAG_NORMAL_MAP, 0, 0, 0, sphip_set_normal_map },
	{ "set_uv", SPHIP_FLAG_TEXTURE | SPHIP_FLAG_NORMAL_MAP, 6, "UV table", sphip_set_uv, 0 },      // the one UV table addresses the atlas and the normal map
};

struct hip_r : public basic_renderer {
	sphip_t* ctx;
	std::string desc;
	unsigned long long seed;
	int flags;
	// scene cache: the reference's GPU peer re-uploads every frame (src/cl_renderer.cpp:210-214); tris/mats are
	// borrowed pointers that may be reused with new contents, so the key is a content hash, not the address
	unsigned long long scene_hash;
	size_t scene_n;
	sphip_stats stats;
	bool have_stats;
	// progressive mode (set_progressive): render() continues the accumulation while the viewport rays (or, for
	// render_own_viewport, the camera), the scene, the seed and the flags are those it was begun with; otherwise it begins anew
	bool progressive;
	bool acc_live, acc_cam;
	std::vector<geom::ray> acc_rays;
	sphip_camera acc_camera;
	size_t acc_w, acc_h, acc_scene_n;
	unsigned long long acc_scene_hash, acc_seed;
	int acc_flags;
	// adaptive sampling (set_adaptive) of the progressive mode: adp.rel_error < 0 is off
	sphip_adaptive adp;
	// denoising (set_denoise) of the progressive mode; raw: the last step's image before the filter
	bool dn_on;
	sphip_denoise dn;
	scene::bitmap raw;
	bool have_raw;
	// per-sample camera rays (set_camera_samples, set_lens): SPHIP_FLAG_CAMERA_SAMPLES on the camera path (render_own_viewport) only;
	// the lens is the context's, and the one an accumulation was begun with joins its key
	bool cam_samples;
	sphip_lens lens, acc_lens;
	// temporal reprojection (set_reproject) of the progressive mode on the camera path: a camera move keeps the accumulation as history
	// (sphip_accum_reproject) where it would begin anew; rp_moves: the moves reprojected so far, which key the seeds of the new samples
	bool rp_on;
	sphip_reproject rp;
	unsigned long long rp_moves;
	// display transform (set_display) of the progressive mode: the bitmap of every step is sphip_accum_display's (of the denoised image
	// with set_denoise); dp_meter: the exposure is metered from the image; dp_exposure: the exposure the last step used
	bool dp_on, dp_meter;
	sphip_display dp;
	sphip_metering dp_m;
	float dp_exposure;
	struct part { std::vector<float> v; uint32_t w, h; part() : w(0), h(0) {} };      // empty: not set; w, h: an image's size
	part parts[N_PARTS];

	// ids == 0: every visible GPU of the node (or the list in SPATH_HIP_DEVICES) behind this one renderer object: the frame is
	// dealt to them as interleaved pixel-row tiles and reassembled on the first (include/spath_hip.h: sphip_create_multi)
	hip_r(const int x, const int y, const int* ids, const int n_ids) : basic_renderer(x, y), ctx(0), seed(1), flags(0), scene_hash(0), scene_n(0), have_stats(false),
	                                                                   progressive(false), acc_live(false), acc_cam(false), acc_w(0), acc_h(0), acc_scene_n(0),
	                                                                   acc_scene_hash(0), acc_seed(0), acc_flags(0), dn_on(false), have_raw(false),
	                                                                   cam_samples(false), rp_on(false), rp_moves(0), dp_on(false), dp_meter(false), dp_exposure(1.0f) {
		std::memset(&rp, 0, sizeof rp);
		std::memset(&dp, 0, sizeof dp);
		std::memset(&dp_m, 0, sizeof dp_m);
		std::memset(&acc_camera, 0, sizeof acc_camera);
		std::memset(&lens, 0, sizeof lens);
		std::memset(&acc_lens, 0, sizeof acc_lens);
		std::memset(&dn, 0, sizeof dn);
		std::memset(&adp, 0, sizeof adp);
		adp.rel_error = -1.0;
		if (sphip_create_multi(ids, n_ids, &ctx) != SPHIP_OK)
			throw std::runtime_error(std::string("hip_renderer: ") + sphip_last_error(0));
		desc = sphip_description(ctx);
		std::memset(&stats, 0, sizeof stats);
	}

	virtual ~hip_r() { sphip_destroy(ctx); }

	virtual const char* get_description(void) const { return desc.c_str(); }

	void check(int rc, const char* what) {
		if (rc != SPHIP_OK) throw std::runtime_error(std::string("hip_renderer: ") + what + ": " + sphip_last_error(ctx));
	}

	static unsigned long long fnv(const void* p, size_t n, unsigned long long h) {
		const unsigned char* b = (const unsigned char*)p;
		for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
		return h;
	}

	void upload_scene(const geom::triangle* tris, const scene::material* mats, const size_t n_tris) {
		unsigned long long h = fnv(tris, n_tris * sizeof(geom::triangle), 1469598103934665603ull);
		h = fnv(mats, n_tris * sizeof(scene::material), h);
		for (int i = 0; i < N_PARTS; ++i) {
			const part& q = parts[i];
			if (q.v.empty()) continue;
			if (part_rules[i].floats && q.v.size() != n_tris * part_rules[i].floats)
				throw std::runtime_error(std::string("hip_renderer: the ") + part_rules[i].noun + " and the scene differ in size");
			h = fnv(&q.w, sizeof q.w, h);
			h = fnv(q.v.data(), q.v.size() * sizeof(float), h);
		}
		if (h != scene_hash || n_tris != scene_n) {
			check(sphip_set_scene(ctx, (const float*)tris, (const float*)mats, n_tris), "set_scene");
			for (int i = 0; i < N_PARTS; ++i) {
				const part& q = parts[i];
				const float* p = q.v.empty() ? 0 : q.v.data();
				if (part_rules[i].set_image) check(part_rules[i].set_image(ctx, p, q.w, q.h), part_rules[i].what);     // sent, or cleared, every time
				else if (p) check(part_rules[i].set_table(ctx, p), part_rules[i].what);
			}
			scene_hash = h; scene_n = n_tris;
		}
	}

	// the camera as the C ABI wants it; the trig values are recomputed with the same float std::cos/std::sin calls the
	// reference's camera makes (src/view.h:77-80,87-92) -- its cached copies are private
	sphip_camera camera_args() const {
		sphip_camera c;
		c.pos[0] = vc.pos.x; c.pos[1] = vc.pos.y; c.pos[2] = vc.pos.z;
		c.cos_y = std::cos(vc.angle.y); c.sin_y = std::sin(vc.angle.y);
		c.cos_x = std::cos(vc.angle.x); c.sin_x = std::sin(vc.angle.x);
		c.focal = vc.focal;
		c.res_x = (uint32_t)vc.res_x; c.res_y = (uint32_t)vc.res_y;
		return c;
	}

	bool same_accumulation(size_t w, size_t h, int f) const {
		return acc_live && acc_w == w && acc_h == h && acc_scene_hash == scene_hash && acc_scene_n == scene_n && acc_seed == seed && acc_flags == f;
	}

	void begin(const float* rays, const sphip_camera* cam, size_t w, size_t h, int flags) {
		have_raw = false;
		if (adp.rel_error >= 0.0) check(sphip_accum_begin_adaptive(ctx, rays, cam, w, h, seed, flags, &adp), "accum_begin_adaptive");
		else if (dn_on && !rp_on) {                // with reprojection on the accumulation stays plain: the filter runs without the variance
			sphip_adaptive never;                 // the variance for the filter, the image of a plain accumulation
			std::memset(&never, 0, sizeof never);
			never.min_samples = 0xffffffffu;
			check(sphip_accum_begin_adaptive(ctx, rays, cam, w, h, seed, flags, &never), "accum_begin_adaptive");
		} else check(sphip_accum_begin(ctx, rays, cam, w, h, seed, flags), "accum_begin");
	}

	// one progressive step of n_samples (the accumulation begun or continued by the caller) into out
	void accum_step(const size_t n_samples, scene::bitmap& out) {
		acc_live = false;                  // a failed step ends the accumulation on the library's side too
		check(sphip_accum_step(ctx, n_samples, (uint8_t*)out.values.data(), 0, 0), "accum_step");
		acc_live = true;
		have_stats = sphip_get_stats(ctx, &stats) == SPHIP_OK;
		if (dn_on) {
			raw = out;
			have_raw = true;
		}
		if (dp_on) check(sphip_accum_display(ctx, &dp, dp_meter ? &dp_m : 0, dn_on ? &dn : 0, (uint8_t*)out.values.data(), 0, &dp_exposure), "accum_display");
		else if (dn_on) check(sphip_accum_denoise(ctx, &dn, (uint8_t*)out.values.data(), 0), "accum_denoise");
	}

	void frame_own_viewport(const geom::triangle* tris, const scene::material* mats, const size_t n_tris, const size_t n_samples,
	                        scene::bitmap& out, const int mode) {
		upload_scene(tris, mats, n_tris);
		out.res_x = vc.res_x;
		out.res_y = vc.res_y;
		out.values.resize(out.res_x * out.res_y);
		const sphip_camera c = camera_args();
		const int f = (cam_samples ? (flags | SPHIP_FLAG_CAMERA_SAMPLES) : flags) | table_flags(mode);
		if (progressive && mode == SPHIP_MODE_PT) {
			const bool same = same_accumulation(c.res_x, c.res_y, f) && acc_cam && std::memcmp(&lens, &acc_lens, sizeof lens) == 0;
			if (same && std::memcmp(&c, &acc_camera, sizeof c) == 0) {
				// the view stands still: the accumulation goes on
			} else if (same && rp_on && adp.rel_error < 0.0) {
				// only the camera moved (set_delta_mov / set_delta_rot / set_delta_focal): the accumulation becomes the new view's history
				acc_live = false;
				have_raw = false;
				++rp_moves;
				check(sphip_accum_reproject(ctx, &c, seed + rp_moves, &rp), "accum_reproject");
				acc_live = true;
				acc_camera = c;
			} else {
				acc_live = false;
				begin(0, &c, c.res_x, c.res_y, f);
				begun(c.res_x, c.res_y, true, f);
				acc_camera = c;
				acc_lens = lens;
				acc_rays.clear();
			}
			accum_step(n_samples, out);
			return;
		}
		check(sphip_render_camera(ctx, &c, n_samples, seed, mode, f, (uint8_t*)out.values.data(), 0), "render_camera");
		have_stats = sphip_get_stats(ctx, &stats) == SPHIP_OK;
	}

	int table_flags(const int mode) const {              // the flags whose tables and images are all set
		if (mode != SPHIP_MODE_PT) return 0;
		int on = 0, off = 0;
		for (int i = 0; i < N_PARTS; ++i) (parts[i].v.empty() ? off : on) |= part_rules[i].flag;
		return on & ~off;                                             // SPHIP_FLAG_TEXTURE needs both the atlas and the UV table
	}

	void frame(const view::viewport& vp, const geom::triangle* tris, const scene::material* mats, const size_t n_tris,
	           const size_t n_samples, scene::bitmap& out, const int mode) {
		upload_scene(tris, mats, n_tris);
		const int flags = this->flags | table_flags(mode);
		// first ensure that the bitmap is of correct size (src/cpu_renderer.cpp:120-122)
		out.res_x = vp.res_x;
		out.res_y = vp.res_y;
		out.values.resize(out.res_x * out.res_y);
		if (vp.rays.size() != out.values.size()) throw std::runtime_error("hip_renderer: viewport size and ray count disagree");
		if (progressive && mode == SPHIP_MODE_PT) {
			// the rays are compared bit for bit with those the accumulation was begun with
			if (!(same_accumulation(vp.res_x, vp.res_y, flags) && !acc_cam && acc_rays.size() == vp.rays.size() &&
			      std::memcmp(acc_rays.data(), vp.rays.data(), vp.rays.size() * sizeof(geom::ray)) == 0)) {
				acc_live = false;
				begin((const float*)vp.rays.data(), 0, vp.res_x, vp.res_y, flags);
				begun(vp.res_x, vp.res_y, false, flags);
				acc_rays.assign(vp.rays.begin(), vp.rays.end());
			}
			accum_step(n_samples, out);
			return;
		}
		check(sphip_render(ctx, (const float*)vp.rays.data(), vp.res_x, vp.res_y, n_samples, seed, mode, flags,
		                   (uint8_t*)out.values.data(), 0), "render");
		have_stats = sphip_get_stats(ctx, &stats) == SPHIP_OK;
	}

	void begun(size_t w, size_t h, bool cam, int f) {
		acc_live = true; acc_cam = cam;
		acc_w = w; acc_h = h;
		acc_scene_hash = scene_hash; acc_scene_n = scene_n;
		acc_seed = seed; acc_flags = f;
	}

	virtual void render_flat(const view::viewport& vp, const geom::triangle* tris, const scene::material* mats, const size_t n_tris, const size_t n_samples, scene::bitmap& out) {
		frame(vp, tris, mats, n_tris, n_samples ? n_samples : 1, out, SPHIP_MODE_FLAT);     // n_samples unused (src/cpu_renderer.cpp:81)
	}

	virtual void render(const view::viewport& vp, const geom::triangle* tris, const scene::material* mats, const size_t n_tris, const size_t n_samples, scene::bitmap& out) {
		frame(vp, tris, mats, n_tris, n_samples, out, SPHIP_MODE_PT);
	}
};

} // namespace

namespace hip_renderer {
	// One GPU: device 0, or the devices listed in SPATH_HIP_DEVICES.  Several GPUs behind one renderer are opt-in (get_on /
	// get_all_devices): the cross-device exchange has not run on a multi-GPU node yet.
	scene::renderer* get(const int w, const int h) {
		if (std::getenv("SPATH_HIP_DEVICES")) return new hip_r(w, h, 0, 0);
		const int first = 0;
		return new hip_r(w, h, &first, 1);
	}

	scene::renderer* get_all_devices(const int w, const int h) {
		return new hip_r(w, h, 0, 0);
	}

	scene::renderer* get_on(const int w, const int h, const int* device_ids, const int n_devices) {
		return new hip_r(w, h, device_ids, n_devices);
	}

	int device_count(scene::renderer* r) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		return p ? sphip_device_count(p->ctx) : 0;
	}

	void set_seed(scene::renderer* r, unsigned long long seed) {
		if (hip_r* p = dynamic_cast<hip_r*>(r)) p->seed = seed;
	}

	void set_flags(scene::renderer* r, int flags) {
		if (hip_r* p = dynamic_cast<hip_r*>(r)) p->flags = flags;
	}

	void set_nee(scene::renderer* r, bool on) {
		if (hip_r* p = dynamic_cast<hip_r*>(r)) p->flags = on ? (p->flags | SPHIP_FLAG_NEE) : (p->flags & ~SPHIP_FLAG_NEE);
	}

	void set_mis(scene::renderer* r, bool on) {
		const int f = SPHIP_FLAG_NEE | SPHIP_FLAG_MIS;
		if (hip_r* p = dynamic_cast<hip_r*>(r)) p->flags = on ? (p->flags | f) : (p->flags & ~SPHIP_FLAG_MIS);
	}

	void set_camera_samples(scene::renderer* r, bool on) {
		if (hip_r* p = dynamic_cast<hip_r*>(r)) p->cam_samples = on;
	}

	// one part from the caller's `count` floats (copied), or none with src == NULL or count == 0
	static void keep(scene::renderer* r, part_id id, const float* src, size_t count, uint32_t w = 0, uint32_t h = 0) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		hip_r::part& q = p->parts[id];
		if (src && count) { q.v.assign(src, src + count); q.w = w; q.h = h; }
		else { q.v.clear(); q.w = q.h = 0; }
		p->scene_n = 0;                    // the next frame uploads the scene again, and the table, map or atlas (or none) with it
	}
	static void keep_table(scene::renderer* r, part_id id, const float* rows, size_t n_tris) { keep(r, id, rows, n_tris * part_rules[id].floats); }

	void set_specular(scene::renderer* r, const float* spec, size_t n_tris) { keep_table(r, P_SPEC, spec, n_tris); }
	void set_vertex_normals(scene::renderer* r, const float* vn, size_t n_tris) { keep_table(r, P_VNORM, vn, n_tris); }
	void set_dielectric(scene::renderer* r, const float* glass, size_t n_tris) { keep_table(r, P_GLASS, glass, n_tris); }
	void set_roughness(scene::renderer* r, const float* alpha, size_t n_tris) { keep_table(r, P_ROUGH, alpha, n_tris); }
	void set_uv(scene::renderer* r, const float* uv, size_t n_tris) { keep_table(r, P_UV, uv, n_tris); }
	void set_environment(scene::renderer* r, const float* texels, uint32_t n) { keep(r, P_ENV, texels, (size_t)n * n * 3, n, n); }
	void set_texture(scene::renderer* r, const float* texels, uint32_t tw, uint32_t th) { keep(r, P_TEX, texels, (size_t)tw * th * 3, tw, th); }
	void set_normal_map(scene::renderer* r, const float* texels, uint32_t nw, uint32_t nh) { keep(r, P_NMAP, texels, (size_t)nw * nh * 3, nw, nh); }

	void set_lens(scene::renderer* r, float aperture, float focus_dist) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		sphip_lens l;
		std::memset(&l, 0, sizeof l);
		l.aperture = aperture;
		l.focus_dist = focus_dist;
		p->check(sphip_set_lens(p->ctx, &l), "set_lens");
		p->lens = l;
	}

	void set_progressive(scene::renderer* r, bool on) {
		if (hip_r* p = dynamic_cast<hip_r*>(r)) { p->progressive = on; p->acc_live = false; }
	}

	void set_adaptive(scene::renderer* r, double t, double floor, unsigned min_samples) {
		if (hip_r* p = dynamic_cast<hip_r*>(r)) {
			if (t >= 0.0 && p->rp_on) throw std::runtime_error("hip_renderer: set_adaptive: sphip_accum_reproject needs a plain accumulation, not an adaptive one");
			p->adp.rel_error = t < 0.0 ? -1.0 : t;
			p->adp.floor = floor;
			p->adp.min_samples = min_samples;
			p->adp.reserved = 0;
			p->acc_live = false;
		}
	}

	void set_reproject(scene::renderer* r, const sphip_reproject* p) {
		hip_r* q = dynamic_cast<hip_r*>(r);
		if (!q) return;
		if (p && q->adp.rel_error >= 0.0)          // what the library answers to sphip_accum_reproject on an adaptive accumulation
			throw std::runtime_error("hip_renderer: set_reproject: sphip_accum_reproject needs a plain accumulation, not an adaptive one");
		if (q->rp_on != (p != 0) && q->dn_on) q->acc_live = false;     // the rule the accumulation begins with changes
		q->rp_on = p != 0;
		if (p) q->rp = *p;
	}

	void set_denoise(scene::renderer* r, const sphip_denoise* p) {
		if (hip_r* q = dynamic_cast<hip_r*>(r)) {
			if (q->dn_on != (p != 0)) q->acc_live = false;       // the rule the accumulation begins with changes
			q->dn_on = p != 0;
			if (p) q->dn = *p;
			q->have_raw = false;
		}
	}

	void set_display(scene::renderer* r, const sphip_display* p, const sphip_metering* m) {
		if (hip_r* q = dynamic_cast<hip_r*>(r)) {
			q->dp_on = p != 0;                                   // a post-process of each step's image: the accumulation goes on
			q->dp_meter = p != 0 && m != 0;
			if (p) { q->dp = *p; q->dp_exposure = p->exposure; }
			if (q->dp_meter) q->dp_m = *m;
		}
	}

	float display_exposure(scene::renderer* r) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		return p && p->dp_on ? p->dp_exposure : 1.0f;
	}

	const scene::bitmap* raw_bitmap(scene::renderer* r) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		return p && p->have_raw ? &p->raw : 0;
	}

	bool accum_counts(scene::renderer* r, uint32_t* counts, unsigned long long* n_active) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p || !p->acc_live) return false;
		uint64_t na = 0;
		p->check(sphip_accum_counts(p->ctx, counts, &na), "accum_counts");
		if (n_active) *n_active = na;
		return true;
	}

	bool render_own_viewport(scene::renderer* r, const geom::triangle* tris, const scene::material* mats, const size_t n_tris,
	                         const size_t n_samples, scene::bitmap& out, const bool flat) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return false;
		p->frame_own_viewport(tris, mats, n_tris, n_samples ? n_samples : 1, out, flat ? SPHIP_MODE_FLAT : SPHIP_MODE_PT);
		return true;
	}

	bool last_stats(scene::renderer* r, double* kernel_ms, unsigned long long* scans) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p || !p->have_stats) return false;
		if (kernel_ms) *kernel_ms = p->stats.kernel_ms;
		if (scans) *scans = p->stats.scans_executed;
		return true;
	}
}
