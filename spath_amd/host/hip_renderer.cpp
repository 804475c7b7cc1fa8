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
	// specular reflection (set_specular): the table goes to the library with every scene upload (sphip_set_scene clears it) and joins
	// the scene's key; while there is one, path-traced frames carry SPHIP_FLAG_SPECULAR
	std::vector<float> spec;
	// smooth shading (set_vertex_normals): likewise, 9 floats per triangle and SPHIP_FLAG_SMOOTH
	std::vector<float> vnorm;
	// transparency (set_dielectric): likewise, 4 floats per triangle and SPHIP_FLAG_DIELECTRIC
	std::vector<float> glass;
	// glossy reflection (set_roughness): likewise, 1 float per triangle and SPHIP_FLAG_GLOSSY
	std::vector<float> rough;
	// environment lighting (set_environment): the map, env_n x env_n x 3 floats, and SPHIP_FLAG_ENVIRONMENT; the library keeps it across
	// scenes, but it travels with the scene upload like the tables so that one key covers everything a frame depends on
	std::vector<float> env;
	uint32_t env_n;
	// textures (set_texture, set_uv): the atlas, tex_w x tex_h x 3 floats, travels like the map; the UV table, 6 floats per triangle,
	// like the tables; SPHIP_FLAG_TEXTURE while both are set
	std::vector<float> tex, uv;
	uint32_t tex_w, tex_h;

	// ids == 0: every visible GPU of the node (or the list in SPATH_HIP_DEVICES) behind this one renderer object: the frame is
	// dealt to them as interleaved pixel-row tiles and reassembled on the first (include/spath_hip.h: sphip_create_multi)
	hip_r(const int x, const int y, const int* ids, const int n_ids) : basic_renderer(x, y), ctx(0), seed(1), flags(0), scene_hash(0), scene_n(0), have_stats(false),
	                                                                   progressive(false), acc_live(false), acc_cam(false), acc_w(0), acc_h(0), acc_scene_n(0),
	                                                                   acc_scene_hash(0), acc_seed(0), acc_flags(0), dn_on(false), have_raw(false),
	                                                                   cam_samples(false), env_n(0), tex_w(0), tex_h(0) {
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
		if (!spec.empty()) {
			if (spec.size() != n_tris * 4) throw std::runtime_error("hip_renderer: the specular table and the scene differ in size");
			h = fnv(spec.data(), spec.size() * sizeof(float), h);
		}
		if (!vnorm.empty()) {
			if (vnorm.size() != n_tris * 9) throw std::runtime_error("hip_renderer: the vertex normals and the scene differ in size");
			h = fnv(vnorm.data(), vnorm.size() * sizeof(float), h);
		}
		if (!glass.empty()) {
			if (glass.size() != n_tris * 4) throw std::runtime_error("hip_renderer: the dielectric table and the scene differ in size");
			h = fnv(glass.data(), glass.size() * sizeof(float), h);
		}
		if (!rough.empty()) {
			if (rough.size() != n_tris) throw std::runtime_error("hip_renderer: the roughness table and the scene differ in size");
			h = fnv(rough.data(), rough.size() * sizeof(float), h);
		}
		if (!env.empty()) h = fnv(env.data(), env.size() * sizeof(float), h);
		if (!uv.empty()) {
			if (uv.size() != n_tris * 6) throw std::runtime_error("hip_renderer: the UV table and the scene differ in size");
			h = fnv(uv.data(), uv.size() * sizeof(float), h);
		}
		if (!tex.empty()) { h = fnv(&tex_w, sizeof tex_w, h); h = fnv(tex.data(), tex.size() * sizeof(float), h); }
		if (h != scene_hash || n_tris != scene_n) {
			check(sphip_set_scene(ctx, (const float*)tris, (const float*)mats, n_tris), "set_scene");
			check(sphip_set_environment(ctx, env.empty() ? 0 : env.data(), env_n), "set_environment");
			if (!spec.empty()) check(sphip_set_specular(ctx, spec.data()), "set_specular");
			if (!vnorm.empty()) check(sphip_set_vertex_normals(ctx, vnorm.data()), "set_vertex_normals");
			if (!glass.empty()) check(sphip_set_dielectric(ctx, glass.data()), "set_dielectric");
			if (!rough.empty()) check(sphip_set_roughness(ctx, rough.data()), "set_roughness");
			check(sphip_set_texture(ctx, tex.empty() ? 0 : tex.data(), tex_w, tex_h), "set_texture");
			if (!uv.empty()) check(sphip_set_uv(ctx, uv.data()), "set_uv");
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
		else if (dn_on) {
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
			check(sphip_accum_denoise(ctx, &dn, (uint8_t*)out.values.data(), 0), "accum_denoise");
		}
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
			if (!(same_accumulation(c.res_x, c.res_y, f) && acc_cam && std::memcmp(&c, &acc_camera, sizeof c) == 0 &&
			      std::memcmp(&lens, &acc_lens, sizeof lens) == 0)) {
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

	int table_flags(const int mode) const {              // the flags of the tables that are set
		if (mode != SPHIP_MODE_PT) return 0;
		return (!spec.empty() ? SPHIP_FLAG_SPECULAR : 0) | (!vnorm.empty() ? SPHIP_FLAG_SMOOTH : 0) | (!glass.empty() ? SPHIP_FLAG_DIELECTRIC : 0) |
		       (!env.empty() ? SPHIP_FLAG_ENVIRONMENT : 0) | (!rough.empty() ? SPHIP_FLAG_GLOSSY : 0) |
		       (!tex.empty() && !uv.empty() ? SPHIP_FLAG_TEXTURE : 0);
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

	void set_specular(scene::renderer* r, const float* spec, size_t n_tris) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		if (spec && n_tris) p->spec.assign(spec, spec + n_tris * 4);
		else p->spec.clear();
		p->scene_n = 0;                    // the next frame uploads the scene again, and the table (or none) with it
	}

	void set_dielectric(scene::renderer* r, const float* glass, size_t n_tris) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		if (glass && n_tris) p->glass.assign(glass, glass + n_tris * 4);
		else p->glass.clear();
		p->scene_n = 0;                    // the next frame uploads the scene again, and the table (or none) with it
	}

	void set_roughness(scene::renderer* r, const float* alpha, size_t n_tris) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		if (alpha && n_tris) p->rough.assign(alpha, alpha + n_tris);
		else p->rough.clear();
		p->scene_n = 0;                    // the next frame uploads the scene again, and the table (or none) with it
	}

	void set_texture(scene::renderer* r, const float* texels, uint32_t tw, uint32_t th) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		if (texels && tw && th) { p->tex.assign(texels, texels + (size_t)tw * th * 3); p->tex_w = tw; p->tex_h = th; }
		else { p->tex.clear(); p->tex_w = p->tex_h = 0; }
		p->scene_n = 0;                    // the next frame uploads the scene again, and the atlas (or none) with it
	}

	void set_uv(scene::renderer* r, const float* uv, size_t n_tris) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		if (uv && n_tris) p->uv.assign(uv, uv + n_tris * 6);
		else p->uv.clear();
		p->scene_n = 0;                    // the next frame uploads the scene again, and the table (or none) with it
	}

	void set_environment(scene::renderer* r, const float* texels, uint32_t n) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		if (texels && n) { p->env.assign(texels, texels + (size_t)n * n * 3); p->env_n = n; }
		else { p->env.clear(); p->env_n = 0; }
		p->scene_n = 0;                    // the next frame uploads the scene again, and the map (or none) with it
	}

	void set_vertex_normals(scene::renderer* r, const float* vn, size_t n_tris) {
		hip_r* p = dynamic_cast<hip_r*>(r);
		if (!p) return;
		if (vn && n_tris) p->vnorm.assign(vn, vn + n_tris * 9);
		else p->vnorm.clear();
		p->scene_n = 0;                    // the next frame uploads the scene again, and the normals (or none) with it
	}

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
			p->adp.rel_error = t < 0.0 ? -1.0 : t;
			p->adp.floor = floor;
			p->adp.min_samples = min_samples;
			p->adp.reserved = 0;
			p->acc_live = false;
		}
	}

	void set_denoise(scene::renderer* r, const sphip_denoise* p) {
		if (hip_r* q = dynamic_cast<hip_r*>(r)) {
			if (q->dn_on != (p != 0)) q->acc_live = false;       // the rule the accumulation begins with changes
			q->dn_on = p != 0;
			if (p) q->dn = *p;
			q->have_raw = false;
		}
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
