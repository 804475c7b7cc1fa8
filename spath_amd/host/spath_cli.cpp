// Headless front end for the renderer plugin interface: what the reference's GLUT shell does per frame
// (src/main.cpp:70-83: get_viewport -> render / render_flat -> show the bitmap), minus the window.
// Keys of the interactive shell become flags: camera moves (w/a/s/d, mouse -> --mov/--rot/--focal),
// '+'/'-' -> --spp, 'p' -> --mode.  The image goes to a binary PPM or a raw RGBA file.
//
//   spath_cli [--scene default|FILE.bin] [--w 640 --h 480] [--spp 128] [--mode pt|flat]
//             [--mov x y z] [--rot x y z] [--focal f] [--seed n] [--flags n] [--primary-reuse] [--nee] [--mis] [--aa] [--lens A,F] [--spec FILE.bin] [--normals FILE.bin] [--glass FILE.bin] [--rough FILE.bin] [--env FILE.bin] [--tex FILE.bin --uv FILE.bin] [--nmap FILE.bin --uv FILE.bin] [--out image.ppm|image.rgba] [--frames n]
//             [--device-viewport] [--gpus n | --devices 0,1,... | --all-gpus] [--progressive n [--adaptive T[,FLOOR[,MIN]]] [--counts-out f.pgm]
//              [--denoise [ITER[,SIGMA_L[,SIGMA_Z[,NLOG2]]]] [--raw-out FILE]]
//              [--reproject [MAXH[,NMIN[,PTOL]]] --then-move X,Y,Z[,RX,RY] [--spp-after K] [--first-out FILE]]
//              [--display clamp|reinhard|filmic[,WHITE]] [--exposure auto[,KEY[,LOW,HIGH]]|EV] [--srgb]]
// --display CURVE[,WHITE], --exposure auto[,KEY[,LOW,HIGH]] | EV, --srgb: with --progressive, the image of every step goes through the
//   display transform (include/spath_hip.h: sphip_accum_display) instead of the linear clamp.  Any of the three turns it on, starting
//   from the identity (curve clamp, exposure 2^0, linear encoding); each changes its own part: the tone curve (WHITE: Reinhard's white
//   point, default 4), the exposure as 2^EV or metered from each step's image (the library's key and window for what is left out; the
//   exposure used is printed with every step), the sRGB encoding.  With --denoise the filtered image is what is metered and shown
// --reproject [MAXH[,NMIN[,PTOL]]] --then-move X,Y,Z[,RX,RY]: with --progressive (and the device-generated viewport), temporal
//   reprojection (include/spath_hip.h: sphip_accum_reproject; the library's defaults for what is left out): after the --spp samples of
//   the last frame the camera moves by X,Y,Z and turns by RX,RY, the accumulation is reprojected into the new view and --spp-after K
//   (default: one step) more samples are blended with it; --out is then that image, --first-out FILE the first view's
// --progressive n: render the --spp samples of a frame as progressive steps of n samples (the last takes the remainder), the way
//   a viewer refines a still view; prints every step, and the final image is byte-identical to the one rendered in one go
// --adaptive T[,FLOOR[,MIN]]: with --progressive, stop converged pixels after each step (include/spath_hip.h: sphip_adaptive;
//   relative error T, FLOOR default 0.1, MIN default 8 samples); every pixel's image is that of its own sample count.
//   --counts-out: the per-pixel sample counts of the last frame as a 16-bit binary PGM (clamped to 65535)
// --denoise [ITER[,SIGMA_L[,SIGMA_Z[,NLOG2]]]]: with --progressive, the image of every step is the accumulation denoised
//   (include/spath_hip.h: sphip_accum_denoise; the library's defaults for what is left out); --raw-out FILE: the last raw image, in
//   the format --out would use for that name
// --nee: next-event estimation (include/spath_hip.h: SPHIP_FLAG_NEE); combines with --progressive, --adaptive and --denoise
// --mis: next-event estimation with multiple importance sampling (SPHIP_FLAG_NEE | SPHIP_FLAG_MIS); implies --nee
// --aa: per-sample camera rays, box-filtered in the pixel (SPHIP_FLAG_CAMERA_SAMPLES); --lens A,F: a thin lens of aperture A focused at
//   F (sphip_lens; implies --aa).  Both render through the device-generated viewport (as --device-viewport)
// --spec FILE.bin: specular reflection (SPHIP_FLAG_SPECULAR) by the table in FILE.bin, a file of its own beside the scene file
//   ('SPSP', n, n x {ks.r ks.g ks.b p} f32: spath_amd/scene.py write_specular); path tracing only, not with --nee without --mis
// --normals FILE.bin: smooth shading (SPHIP_FLAG_SMOOTH) by the vertex normals in FILE.bin, a file of its own beside the scene file
//   ('SPVN', n, n x {n0.xyz n1.xyz n2.xyz} f32: spath_amd/scene.py write_vertex_normals); path tracing only, not with --nee without --mis
// --glass FILE.bin: transparency (SPHIP_FLAG_DIELECTRIC) by the dielectric table in FILE.bin, a file of its own beside the scene file
//   ('SPDI', n, n x {kt.r kt.g kt.b ior} f32: spath_amd/scene.py write_dielectric); path tracing only, not with --nee without --mis
// --rough FILE.bin: glossy reflection (SPHIP_FLAG_GLOSSY) by the roughness table in FILE.bin, a file of its own beside the scene file
//   ('SPRG', n, n x {alpha} f32: spath_amd/scene.py write_roughness); needs --spec; the flat pass ignores it; not with --nee without --mis
// --tex FILE.bin --uv FILE.bin: textures (SPHIP_FLAG_TEXTURE) by the atlas in the first file (u32 tw, u32 th, then tw x th x {r g b} f32:
//   spath_amd/scene.py write_texture) and the UV table in the second (n_tris x {s0 t0 s1 t1 s2 t2} f32, no header: write_uv); both or
//   neither; the flat pass ignores them; not with --nee without --mis
// --nmap FILE.bin --uv FILE.bin: normal mapping (SPHIP_FLAG_NORMAL_MAP) by the map in the first file ('SPNM', u32 nw, u32 nh, then
//   nw x nh x {x y z} f32, signed: spath_amd/scene.py write_normal_map) over the UV table of --uv, which --tex shares; the flat pass
//   ignores it; not with --nee without --mis
// --env FILE.bin: environment lighting (SPHIP_FLAG_ENVIRONMENT) by the octahedral map in FILE.bin, a file of its own ('SPEN', n,
//   n x n x {r g b} f32: spath_amd/scene.py write_environment); path tracing only, not with --nee without --mis
// --out: .ppm (binary P6), .png (8-bit RGB, stored deflate blocks: no compression library needed), anything else = raw RGBA8
#include "hip_renderer.h"
#include "spath_hip.h"

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <memory>
#include <string>
#include <vector>

namespace {

geom::vec3 sub(const geom::vec3& a, const geom::vec3& b) { return geom::vec3(a.x - b.x, a.y - b.y, a.z - b.z); }

void set_flat_normal(geom::triangle& t) {   // unit((v1-v0) x (v2-v0)), the caller's job in the reference too (main.cpp:214-215)
	const geom::vec3 a = sub(t.v1, t.v0), b = sub(t.v2, t.v0);
	const geom::vec3 c(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
	const real l = std::sqrt(c.x * c.x + c.y * c.y + c.z * c.z);
	t.n = geom::vec3(c.x / l, c.y / l, c.z / l);
}

// the demo scene of the reference (values: SURVEY.md Appendix C): pyramid face, floor, area light, back wall
void default_scene(std::vector<geom::triangle>& t, std::vector<scene::material>& m) {
	static const float v[7][9] = {
		{ 0, 0, 1, 0.5f, -0.5f, 0, -0.5f, -0.5f, 0 },
		{ 20, -1, 20, -20, -1, -20, -20, -1, 20 }, { 20, -1, 20, 20, -1, -20, -20, -1, -20 },
		{ 0.75f, 0.75f, 0.75f, -0.75f, 0.75f, 0.75f, 0.75f, 0.75f, -0.75f }, { -0.75f, 0.75f, 0.75f, -0.75f, 0.75f, -0.75f, 0.75f, 0.75f, -0.75f },
		{ 1.25f, 0.5f, 1, 1.25f, -1, 1, -1.25f, -1, 1 }, { 1.25f, 0.5f, 1, -1.25f, -1, 1, -1.25f, 0.5f, 1 } };
	static const float refl[7][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 1, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 } };
	t.resize(7); m.resize(7);
	for (int i = 0; i < 7; ++i) {
		t[i].v0 = geom::vec3(v[i][0], v[i][1], v[i][2]); t[i].v1 = geom::vec3(v[i][3], v[i][4], v[i][5]); t[i].v2 = geom::vec3(v[i][6], v[i][7], v[i][8]);
		set_flat_normal(t[i]);
		m[i].reflectance_color = geom::vec3(refl[i][0], refl[i][1], refl[i][2]);
		const float e = (i == 3 || i == 4) ? 1.0f : 0.0f;
		m[i].emittance_color = geom::vec3(e, e, e);
	}
}

// ---- minimal PNG writer: 8-bit RGB, filter 0 on every row, zlib stream of STORED deflate blocks (RFC 1950/1951/2083)
uint32_t crc32_of(const unsigned char* p, size_t n, uint32_t crc = 0) {
	static uint32_t tab[256];
	static bool init = false;
	if (!init) { for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; tab[i] = c; } init = true; }
	crc = ~crc;
	for (size_t i = 0; i < n; ++i) crc = tab[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
	return ~crc;
}

void png_chunk(FILE* o, const char* type, const std::vector<unsigned char>& data) {
	unsigned char len[4] = { (unsigned char)(data.size() >> 24), (unsigned char)(data.size() >> 16), (unsigned char)(data.size() >> 8), (unsigned char)data.size() };
	std::fwrite(len, 1, 4, o);
	std::vector<unsigned char> td(type, type + 4);
	td.insert(td.end(), data.begin(), data.end());
	std::fwrite(td.data(), 1, td.size(), o);
	const uint32_t c = crc32_of(td.data(), td.size());
	unsigned char cb[4] = { (unsigned char)(c >> 24), (unsigned char)(c >> 16), (unsigned char)(c >> 8), (unsigned char)c };
	std::fwrite(cb, 1, 4, o);
}

void write_png(FILE* o, const scene::bitmap& bmp) {
	const size_t w = bmp.res_x, h = bmp.res_y;
	std::vector<unsigned char> raw;                       // filter byte + RGB per row (row 0 = top, as stored)
	raw.reserve(h * (1 + 3 * w));
	for (size_t j = 0; j < h; ++j) {
		raw.push_back(0);
		for (size_t i = 0; i < w; ++i) { const scene::RGBA& p = bmp.values[j * w + i]; raw.push_back(p.r); raw.push_back(p.g); raw.push_back(p.b); }
	}
	std::vector<unsigned char> z;
	z.push_back(0x78); z.push_back(0x01);                 // zlib header, no compression
	uint32_t a = 1, b = 0;                                // Adler-32 of the raw data
	for (size_t i = 0; i < raw.size(); ++i) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
	for (size_t pos = 0; pos < raw.size() || pos == 0; ) {
		const size_t n = std::min<size_t>(65535, raw.size() - pos);
		const bool last = pos + n >= raw.size();
		z.push_back(last ? 1 : 0);
		z.push_back((unsigned char)(n & 0xff)); z.push_back((unsigned char)(n >> 8));
		z.push_back((unsigned char)(~n & 0xff)); z.push_back((unsigned char)((~n >> 8) & 0xff));
		z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
		pos += n;
		if (last) break;
	}
	const uint32_t ad = (b << 16) | a;
	z.push_back((unsigned char)(ad >> 24)); z.push_back((unsigned char)(ad >> 16)); z.push_back((unsigned char)(ad >> 8)); z.push_back((unsigned char)ad);
	static const unsigned char sig[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
	std::fwrite(sig, 1, 8, o);
	std::vector<unsigned char> hd = { (unsigned char)(w >> 24), (unsigned char)(w >> 16), (unsigned char)(w >> 8), (unsigned char)w,
	                                  (unsigned char)(h >> 24), (unsigned char)(h >> 16), (unsigned char)(h >> 8), (unsigned char)h, 8, 2, 0, 0, 0 };
	png_chunk(o, "IHDR", hd);
	png_chunk(o, "IDAT", z);
	png_chunk(o, "IEND", std::vector<unsigned char>());
}

bool load_scene(const char* path, std::vector<geom::triangle>& t, std::vector<scene::material>& m) {   // 'SPSC' file of spath_amd/scene.py
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	uint32_t hdr[2];
	bool ok = std::fread(hdr, 4, 2, f) == 2 && hdr[0] == 0x43535053u;
	if (ok) {
		t.resize(hdr[1]); m.resize(hdr[1]);
		ok = std::fread(t.data(), sizeof(geom::triangle), hdr[1], f) == hdr[1] && std::fread(m.data(), sizeof(scene::material), hdr[1], f) == hdr[1];
	}
	std::fclose(f);
	return ok;
}

// a per-triangle table file of spath_amd/scene.py: magic, n, n rows of `row` floats (main's table_files lists them)
bool load_table(const char* path, uint32_t magic, size_t row, std::vector<float>& tab) {
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	uint32_t hdr[2];
	bool ok = std::fread(hdr, 4, 2, f) == 2 && hdr[0] == magic;
	if (ok) {
		tab.resize((size_t)hdr[1] * row);
		ok = std::fread(tab.data(), row * 4, hdr[1], f) == hdr[1];
	}
	std::fclose(f);
	return ok;
}

// an environment map file of spath_amd/scene.py: 'SPEN', n, n * n * 3 f32
bool load_environment(const char* path, std::vector<float>& env, uint32_t& n) {
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	uint32_t hdr[2];
	bool ok = std::fread(hdr, 4, 2, f) == 2 && hdr[0] == 0x4E455053u && hdr[1] >= 1 && hdr[1] <= 2048;
	if (ok) {
		n = hdr[1];
		env.resize((size_t)n * n * 3);
		ok = std::fread(env.data(), 4, env.size(), f) == env.size();
	}
	std::fclose(f);
	return ok;
}

} // namespace

// an atlas file of spath_amd/scene.py: u32 tw, u32 th, tw * th * 3 f32
bool load_texture(const char* path, std::vector<float>& tex, uint32_t& tw, uint32_t& th) {
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	uint32_t hdr[2] = { 0, 0 };
	bool ok = std::fread(hdr, 4, 2, f) == 2 && hdr[0] >= 1 && hdr[0] <= 4096 && hdr[1] >= 1 && hdr[1] <= 4096;
	if (ok) {
		tw = hdr[0]; th = hdr[1];
		tex.resize((size_t)tw * th * 3);
		ok = std::fread(tex.data(), sizeof(float), tex.size(), f) == tex.size();
	}
	std::fclose(f);
	return ok;
}

// a normal map file of spath_amd/scene.py: 'SPNM', then an atlas file's layout
bool load_normal_map(const char* path, std::vector<float>& map, uint32_t& nw, uint32_t& nh) {
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	uint32_t hdr[3] = { 0, 0, 0 };
	bool ok = std::fread(hdr, 4, 3, f) == 3 && hdr[0] == 0x4D4E5053u && hdr[1] >= 1 && hdr[1] <= 4096 && hdr[2] >= 1 && hdr[2] <= 4096;
	if (ok) {
		nw = hdr[1]; nh = hdr[2];
		map.resize((size_t)nw * nh * 3);
		ok = std::fread(map.data(), sizeof(float), map.size(), f) == map.size();
	}
	std::fclose(f);
	return ok;
}

// a UV file of spath_amd/scene.py: n_tris * 6 f32, no header
bool load_uv(const char* path, size_t n_tris, std::vector<float>& uv) {
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	uv.resize(n_tris * 6);
	char extra;
	const bool ok = std::fread(uv.data(), sizeof(float), uv.size(), f) == uv.size() && std::fread(&extra, 1, 1, f) == 0;
	std::fclose(f);
	return ok;
}

int main(int argc, char** argv) {
	try {
		std::string scene_arg = "default", mode = "pt", out_path, spec_arg, normals_arg, glass_arg, env_arg, rough_arg, tex_arg, uv_arg, nmap_arg;
		bool device_viewport = false;
		std::vector<int> devices;                                    // empty: one GPU (hip_renderer::get: device 0 or SPATH_HIP_DEVICES)
		bool all_gpus = false;
		int w = 640, h = 480, frames = 1, flags = 0;                 // window default of the reference (main.cpp:238-239)
		bool nee = false, mis = false, aa = false;
		float lens_a = 0.0f, lens_f = 0.0f;
		size_t spp = 128;                                            // main.cpp:44
		size_t progressive = 0;
		double adp_t = -1.0, adp_floor = 0.1;                        // --adaptive defaults: FLOOR 0.1, MIN 8
		unsigned adp_min = 8;
		std::string counts_path, raw_path;
		bool denoise = false, reproject = false, then_move = false;
		sphip_reproject rp;
		sphip_reproject_defaults(&rp);
		float mv[5] = { 0, 0, 0, 0, 0 };
		size_t spp_after = 0;
		std::string first_path;
		sphip_denoise dn;
		sphip_denoise_defaults(&dn);
		bool display = false, meter = false;
		sphip_display dp;
		sphip_display_defaults(&dp);
		dp.curve = SPHIP_CURVE_CLAMP; dp.encode = SPHIP_ENCODE_LINEAR;  // the identity, until an option changes its part
		sphip_metering mt;
		sphip_metering_defaults(&mt);
		unsigned long long seed = 1;
		std::vector<std::pair<char, geom::vec3> > moves;
		for (int i = 1; i < argc; ++i) {
			const std::string k = argv[i];
			auto need = [&](int n) { if (i + n >= argc) throw std::runtime_error("missing value after " + k); };
			if (k == "--scene") { need(1); scene_arg = argv[++i]; }
			else if (k == "--spec") { need(1); spec_arg = argv[++i]; }
			else if (k == "--normals") { need(1); normals_arg = argv[++i]; }
			else if (k == "--glass") { need(1); glass_arg = argv[++i]; }
			else if (k == "--rough") { need(1); rough_arg = argv[++i]; }
			else if (k == "--env") { need(1); env_arg = argv[++i]; }
			else if (k == "--tex") { need(1); tex_arg = argv[++i]; }
			else if (k == "--uv") { need(1); uv_arg = argv[++i]; }
			else if (k == "--nmap") { need(1); nmap_arg = argv[++i]; }
			else if (k == "--w") { need(1); w = std::atoi(argv[++i]); }
			else if (k == "--h") { need(1); h = std::atoi(argv[++i]); }
			else if (k == "--spp") { need(1); spp = (size_t)std::atoll(argv[++i]); }
			else if (k == "--mode") { need(1); mode = argv[++i]; }
			else if (k == "--seed") { need(1); seed = std::strtoull(argv[++i], 0, 0); }
			else if (k == "--flags") { need(1); flags = std::atoi(argv[++i]); }
			else if (k == "--primary-reuse") flags |= SPHIP_FLAG_PRIMARY_REUSE;   // one primary scan per pixel (identical image)
			else if (k == "--nee") nee = true;                                   // next-event estimation (SPHIP_FLAG_NEE)
			else if (k == "--mis") mis = true;                                   // ... with MIS (SPHIP_FLAG_MIS, implies --nee)
			else if (k == "--aa") aa = true;                                     // per-sample camera rays (SPHIP_FLAG_CAMERA_SAMPLES)
			else if (k == "--lens") {                                            // A,F: thin lens (implies --aa)
				need(1);
				const char* p = argv[++i];
				char* e = 0;
				lens_a = std::strtof(p, &e);
				if (e == p || *e != ',' || !std::isfinite(lens_a) || lens_a < 0.0f) throw std::runtime_error("bad --lens value (A,F: aperture A >= 0, focus distance F > 0)");
				p = e + 1;
				lens_f = std::strtof(p, &e);
				if (e == p || *e || !std::isfinite(lens_f) || !(lens_f > 0.0f)) throw std::runtime_error("bad --lens value (A,F: aperture A >= 0, focus distance F > 0)");
				aa = true;
			}
			else if (k == "--progressive") { need(1); progressive = (size_t)std::atoll(argv[++i]); }
			else if (k == "--adaptive") {
				need(1);
				const char* p = argv[++i];
				char* e = 0;
				adp_t = std::strtod(p, &e);
				if (e == p || adp_t < 0.0) throw std::runtime_error("bad --adaptive value (T[,FLOOR[,MIN]], T >= 0)");
				if (*e == ',') { p = e + 1; adp_floor = std::strtod(p, &e); if (e == p) throw std::runtime_error("bad --adaptive FLOOR"); }
				if (*e == ',') { p = e + 1; adp_min = (unsigned)std::strtoul(p, &e, 10); if (e == p) throw std::runtime_error("bad --adaptive MIN"); }
				if (*e) throw std::runtime_error("bad --adaptive value (T[,FLOOR[,MIN]])");
			}
			else if (k == "--counts-out") { need(1); counts_path = argv[++i]; }
			else if (k == "--denoise") {
				denoise = true;
				if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {     // optional ITER[,SIGMA_L[,SIGMA_Z[,NLOG2]]]
					const char* p = argv[++i];
					char* e = 0;
					const unsigned long it = std::strtoul(p, &e, 10);
					if (e == p || it > 8) throw std::runtime_error("bad --denoise value (ITER[,SIGMA_L[,SIGMA_Z[,NLOG2]]], ITER 0..8)");
					dn.iterations = (uint32_t)it;
					if (*e == ',') { p = e + 1; dn.sigma_lum = std::strtof(p, &e); if (e == p) throw std::runtime_error("bad --denoise SIGMA_L"); }
					if (*e == ',') { p = e + 1; dn.sigma_depth = std::strtof(p, &e); if (e == p) throw std::runtime_error("bad --denoise SIGMA_Z"); }
					if (*e == ',') { p = e + 1; dn.normal_log2 = (uint32_t)std::strtoul(p, &e, 10); if (e == p) throw std::runtime_error("bad --denoise NLOG2"); }
					if (*e) throw std::runtime_error("bad --denoise value (ITER[,SIGMA_L[,SIGMA_Z[,NLOG2]]])");
				}
			}
			else if (k == "--display") {
				need(1);
				display = true;
				const std::string v = argv[++i];
				const size_t comma = v.find(',');
				const std::string curve = v.substr(0, comma);
				if (curve == "clamp") dp.curve = SPHIP_CURVE_CLAMP;
				else if (curve == "reinhard") dp.curve = SPHIP_CURVE_REINHARD;
				else if (curve == "filmic") dp.curve = SPHIP_CURVE_FILMIC;
				else throw std::runtime_error("bad --display value (clamp|reinhard|filmic[,WHITE])");
				if (comma != std::string::npos) {
					const char* p = v.c_str() + comma + 1;
					char* e = 0;
					dp.white = std::strtof(p, &e);
					if (e == p || *e || !std::isfinite(dp.white) || !(dp.white > 0.0f)) throw std::runtime_error("bad --display WHITE (finite, > 0)");
				}
			}
			else if (k == "--exposure") {
				need(1);
				display = true;
				const char* p = argv[++i];
				char* e = 0;
				if (std::strncmp(p, "auto", 4) == 0 && (p[4] == 0 || p[4] == ',')) {
					meter = true;
					e = (char*)p + 4;
					if (*e == ',') { p = e + 1; mt.key = std::strtof(p, &e); if (e == p) throw std::runtime_error("bad --exposure KEY"); }
					if (*e == ',') {
						p = e + 1; mt.low = std::strtof(p, &e);
						if (e == p || *e != ',') throw std::runtime_error("bad --exposure value (auto[,KEY[,LOW,HIGH]]: LOW and HIGH go together)");
						p = e + 1; mt.high = std::strtof(p, &e);
						if (e == p) throw std::runtime_error("bad --exposure HIGH");
					}
					if (*e) throw std::runtime_error("bad --exposure value (auto[,KEY[,LOW,HIGH]] | EV)");
				} else {
					const float ev = std::strtof(p, &e);
					if (e == p || *e || !std::isfinite(ev)) throw std::runtime_error("bad --exposure value (auto[,KEY[,LOW,HIGH]] | EV)");
					meter = false;
					dp.exposure = std::exp2(ev);
				}
			}
			else if (k == "--srgb") { display = true; dp.encode = SPHIP_ENCODE_SRGB; }
			else if (k == "--raw-out") { need(1); raw_path = argv[++i]; }
			else if (k == "--reproject") {
				reproject = true;
				if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {     // optional MAXH[,NMIN[,PTOL]]
					const char* p = argv[++i];
					char* e = 0;
					rp.max_history = std::strtof(p, &e);
					if (e == p) throw std::runtime_error("bad --reproject value (MAXH[,NMIN[,PTOL]])");
					if (*e == ',') { p = e + 1; rp.normal_min = std::strtof(p, &e); if (e == p) throw std::runtime_error("bad --reproject NMIN"); }
					if (*e == ',') { p = e + 1; rp.plane_tol = std::strtof(p, &e); if (e == p) throw std::runtime_error("bad --reproject PTOL"); }
					if (*e) throw std::runtime_error("bad --reproject value (MAXH[,NMIN[,PTOL]])");
				}
			}
			else if (k == "--then-move") {
				need(1);
				then_move = true;
				const char* p = argv[++i];
				int got = 0;
				for (; got < 5; ++got) {
					char* e = 0;
					mv[got] = std::strtof(p, &e);
					if (e == p) throw std::runtime_error("bad --then-move value (X,Y,Z[,RX,RY])");
					p = e;
					if (*p != ',') { ++got; break; }
					++p;
				}
				if (*p || (got != 3 && got != 5)) throw std::runtime_error("bad --then-move value (X,Y,Z[,RX,RY])");
			}
			else if (k == "--spp-after") { need(1); spp_after = (size_t)std::atoll(argv[++i]); }
			else if (k == "--first-out") { need(1); first_path = argv[++i]; }
			else if (k == "--frames") { need(1); frames = std::atoi(argv[++i]); }
			else if (k == "--out") { need(1); out_path = argv[++i]; }
			else if (k == "--device-viewport") device_viewport = true;
			else if (k == "--all-gpus") all_gpus = true;
			else if (k == "--gpus") { need(1); const int n = std::atoi(argv[++i]); devices.clear(); for (int d = 0; d < n; ++d) devices.push_back(d); }
			else if (k == "--devices") { need(1); devices.clear(); for (const char* p = argv[++i]; *p;) { char* e = 0; devices.push_back((int)std::strtol(p, &e, 10)); if (e == p) throw std::runtime_error("bad --devices list"); p = *e ? e + 1 : e; } }
			else if (k == "--mov" || k == "--rot") { need(3); moves.push_back(std::make_pair(k[2], geom::vec3(std::atof(argv[i + 1]), std::atof(argv[i + 2]), std::atof(argv[i + 3])))); i += 3; }
			else if (k == "--focal") { need(1); moves.push_back(std::make_pair('f', geom::vec3(std::atof(argv[++i]), 0, 0))); }
			else throw std::runtime_error("unknown argument " + k);
		}
		if (denoise && !(progressive && mode == "pt")) throw std::runtime_error("--denoise needs --progressive n and --mode pt");
		if (display && !(progressive && mode == "pt")) throw std::runtime_error("--display, --exposure and --srgb need --progressive n and --mode pt");
		if (!raw_path.empty() && !denoise) throw std::runtime_error("--raw-out needs --denoise");
		if (reproject != then_move) throw std::runtime_error("--reproject and --then-move go together");
		if (reproject && !(progressive && mode == "pt")) throw std::runtime_error("--reproject needs --progressive n and --mode pt");
		if ((spp_after || !first_path.empty()) && !reproject) throw std::runtime_error("--spp-after and --first-out need --reproject");
		if (reproject) device_viewport = true;                          // the reprojection needs the camera
		if (!env_arg.empty() && mode != "pt") throw std::runtime_error("--env needs --mode pt");
		if (!env_arg.empty() && nee && !mis) throw std::runtime_error("--env works with the plain estimator and with --mis, not with --nee alone");
		if (!nmap_arg.empty() && uv_arg.empty()) throw std::runtime_error("--nmap needs --uv (the UV table addresses the normal map)");
		if (!nmap_arg.empty() && nee && !mis) throw std::runtime_error("--nmap works with the plain estimator and with --mis, not with --nee alone");
		if (tex_arg.empty() != uv_arg.empty() && (nmap_arg.empty() || !tex_arg.empty())) throw std::runtime_error("--tex and --uv go together (the atlas and the UV table)");
		if (!tex_arg.empty() && nee && !mis) throw std::runtime_error("--tex works with the plain estimator and with --mis, not with --nee alone");
		if (!rough_arg.empty() && spec_arg.empty()) throw std::runtime_error("--rough needs --spec (it roughens the mirror lobe of the specular table)");
		if (!rough_arg.empty() && nee && !mis) throw std::runtime_error("--rough works with the plain estimator and with --mis, not with --nee alone");
		std::vector<geom::triangle> tris;
		std::vector<scene::material> mats;
		if (scene_arg == "default") default_scene(tris, mats);
		else if (!load_scene(scene_arg.c_str(), tris, mats)) throw std::runtime_error("cannot read scene file " + scene_arg);

		std::unique_ptr<scene::renderer> r(!devices.empty() ? hip_renderer::get_on(w, h, devices.data(), (int)devices.size())      // main.cpp:242-244
		                                   : all_gpus ? hip_renderer::get_all_devices(w, h) : hip_renderer::get(w, h));
		hip_renderer::set_seed(r.get(), seed);
		hip_renderer::set_flags(r.get(), flags);
		hip_renderer::set_nee(r.get(), nee);
		if (mis) hip_renderer::set_mis(r.get(), true);
		hip_renderer::set_camera_samples(r.get(), aa);
		// the table files that carry a magic ('SPSP', 'SPVN', 'SPDI', 'SPRG'): the argument, the magic, floats per triangle, the noun, the setter
		const struct { const std::string& arg; uint32_t magic; size_t row; const char* noun; void (*set)(scene::renderer*, const float*, size_t); } table_files[] = {
			{ spec_arg, 0x50535053u, 4, "specular", hip_renderer::set_specular },
			{ normals_arg, 0x4E565053u, 9, "vertex-normal", hip_renderer::set_vertex_normals },
			{ glass_arg, 0x49445053u, 4, "dielectric", hip_renderer::set_dielectric },
			{ rough_arg, 0x47525053u, 1, "roughness", hip_renderer::set_roughness },
		};
		for (const auto& t : table_files) {
			if (t.arg.empty()) continue;
			std::vector<float> tab;
			if (!load_table(t.arg.c_str(), t.magic, t.row, tab)) throw std::runtime_error(std::string("cannot read ") + t.noun + " file " + t.arg);
			if (tab.size() != tris.size() * t.row) throw std::runtime_error(std::string("the ") + t.noun + " file " + t.arg + " and the scene differ in size");
			t.set(r.get(), tab.data(), tris.size());
		}
		if (!tex_arg.empty()) {
			std::vector<float> tex;
			uint32_t tw = 0, th = 0;
			if (!load_texture(tex_arg.c_str(), tex, tw, th)) throw std::runtime_error("cannot read atlas file " + tex_arg);
			hip_renderer::set_texture(r.get(), tex.data(), tw, th);
		}
		if (!nmap_arg.empty()) {
			std::vector<float> map;
			uint32_t nw = 0, nh = 0;
			if (!load_normal_map(nmap_arg.c_str(), map, nw, nh)) throw std::runtime_error("cannot read normal map file " + nmap_arg);
			hip_renderer::set_normal_map(r.get(), map.data(), nw, nh);
		}
		if (!uv_arg.empty()) {
			std::vector<float> uv;
			if (!load_uv(uv_arg.c_str(), tris.size(), uv)) throw std::runtime_error("cannot read UV file " + uv_arg + " (n_tris x 6 floats for this scene)");
			hip_renderer::set_uv(r.get(), uv.data(), tris.size());
		}
		if (!env_arg.empty()) {
			std::vector<float> env;
			uint32_t env_n = 0;
			if (!load_environment(env_arg.c_str(), env, env_n)) throw std::runtime_error("cannot read environment file " + env_arg);
			hip_renderer::set_environment(r.get(), env.data(), env_n);
		}
		hip_renderer::set_lens(r.get(), lens_a, lens_f);
		if (aa) device_viewport = true;                                  // camera samples live on the camera path
		if (adp_t >= 0.0 && !(progressive && mode == "pt")) throw std::runtime_error("--adaptive needs --progressive n and --mode pt");
		if (!counts_path.empty() && !(progressive && mode == "pt")) throw std::runtime_error("--counts-out needs --progressive n and --mode pt");
		hip_renderer::set_adaptive(r.get(), adp_t, adp_floor, adp_min);
		hip_renderer::set_denoise(r.get(), denoise ? &dn : 0);
		hip_renderer::set_reproject(r.get(), reproject ? &rp : 0);       // throws with --adaptive: the library's refusal
		hip_renderer::set_display(r.get(), display ? &dp : 0, meter ? &mt : 0);
		std::printf("Current renderer: %s [%d device(s)]\n", r->get_description(), hip_renderer::device_count(r.get()));     // main.cpp:30-32
		for (size_t k = 0; k < moves.size(); ++k) {
			if (moves[k].first == 'm') r->set_delta_mov(moves[k].second);
			else if (moves[k].first == 'r') r->set_delta_rot(moves[k].second);
			else r->set_delta_focal(moves[k].second.x);
		}
		view::viewport vp;
		scene::bitmap bmp;
		for (int f = 0; f < frames; ++f) {
			const auto t0 = std::chrono::steady_clock::now();
			if (progressive && mode == "pt") {
				hip_renderer::set_progressive(r.get(), true);            // every frame begins a new accumulation
				if (!device_viewport) r->get_viewport(vp);
				for (size_t done = 0, step = 0; done < spp; ++step) {
					const size_t n = std::min(progressive, spp - done);
					if (device_viewport) hip_renderer::render_own_viewport(r.get(), tris.data(), mats.data(), tris.size(), n, bmp, false);
					else r->render(vp, tris.data(), mats.data(), tris.size(), n, bmp);
					done += n;
					double kms = 0;
					hip_renderer::last_stats(r.get(), &kms, 0);
					unsigned long long active = 0;
					if (display) std::printf("  step %zu: exposure %.9g\n", step, (double)hip_renderer::display_exposure(r.get()));
					if (adp_t >= 0.0 && hip_renderer::accum_counts(r.get(), 0, &active))
						std::printf("  step %zu: %zu spp (%zu so far), kernel %.3f ms, %llu pixels active\n", step, n, done, kms, active);
					else std::printf("  step %zu: %zu spp (%zu so far), kernel %.3f ms\n", step, n, done, kms);
				}
			} else if (device_viewport) {                                       // rays generated on the GPU, never uploaded
				hip_renderer::render_own_viewport(r.get(), tris.data(), mats.data(), tris.size(), spp, bmp, mode != "pt");
			} else {
				r->get_viewport(vp);                                     // main.cpp:74
				if (mode == "pt") r->render(vp, tris.data(), mats.data(), tris.size(), spp, bmp);
				else r->render_flat(vp, tris.data(), mats.data(), tris.size(), spp, bmp);
			}
			const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			double kms = 0; unsigned long long scans = 0;
			hip_renderer::last_stats(r.get(), &kms, &scans);
			std::printf("Done (%.3fs) frame %d: %dx%d, %zu spp, %zu triangles, kernel %.3f ms, %llu scans, %.1f Mray/s nominal\n", s, f, w, h,
			            spp, tris.size(), kms, scans, mode == "pt" ? (double)w * h * spp * 5 / s / 1e6 : (double)w * h / s / 1e6);
		}
		auto write_image = [](const std::string& path, const scene::bitmap& b) {
			FILE* o = std::fopen(path.c_str(), "wb");
			if (!o) throw std::runtime_error("cannot write " + path);
			if (path.size() > 4 && path.substr(path.size() - 4) == ".ppm") {
				std::fprintf(o, "P6\n%zu %zu\n255\n", b.res_x, b.res_y);
				for (size_t i = 0; i < b.values.size(); ++i) std::fwrite(&b.values[i], 1, 3, o);   // row 0 = top, as stored
			} else if (path.size() > 4 && path.substr(path.size() - 4) == ".png") {
				write_png(o, b);
			} else {
				std::fwrite(b.values.data(), sizeof(scene::RGBA), b.values.size(), o);
			}
			std::fclose(o);
		};
		if (reproject) {                                                // the camera moves, the accumulation follows it
			if (!first_path.empty()) write_image(first_path, bmp);
			r->set_delta_mov(geom::vec3(mv[0], mv[1], mv[2]));
			if (mv[3] != 0.0f || mv[4] != 0.0f) r->set_delta_rot(geom::vec3(mv[3], mv[4], 0));
			const size_t more = spp_after ? spp_after : progressive;
			for (size_t done = 0, step = 0; done < more; ++step) {
				const size_t n = std::min(progressive, more - done);
				hip_renderer::render_own_viewport(r.get(), tris.data(), mats.data(), tris.size(), n, bmp, false);
				done += n;
				double kms = 0;
				hip_renderer::last_stats(r.get(), &kms, 0);
				std::printf("  after the move, step %zu: %zu spp (%zu new so far), kernel %.3f ms\n", step, n, done, kms);
				if (display) std::printf("  after the move, step %zu: exposure %.9g\n", step, (double)hip_renderer::display_exposure(r.get()));
			}
		}
		if (!out_path.empty()) write_image(out_path, bmp);
		if (!raw_path.empty()) {
			const scene::bitmap* raw = hip_renderer::raw_bitmap(r.get());
			if (!raw) throw std::runtime_error("no raw image to write");
			write_image(raw_path, *raw);
		}
		if (!counts_path.empty()) {
			std::vector<uint32_t> counts(bmp.values.size());
			if (!hip_renderer::accum_counts(r.get(), counts.data(), 0)) throw std::runtime_error("no accumulation to read the counts of");
			FILE* o = std::fopen(counts_path.c_str(), "wb");
			if (!o) throw std::runtime_error("cannot write " + counts_path);
			std::fprintf(o, "P5\n%zu %zu\n65535\n", bmp.res_x, bmp.res_y);
			for (size_t i = 0; i < counts.size(); ++i) {                 // 16-bit PGM: big-endian samples
				const unsigned v = counts[i] < 65535u ? counts[i] : 65535u;
				const unsigned char b[2] = { (unsigned char)(v >> 8), (unsigned char)(v & 0xff) };
				std::fwrite(b, 1, 2, o);
			}
			std::fclose(o);
		}
	} catch (const std::exception& e) {
		std::fprintf(stderr, "Exception: %s\n", e.what());               // main.cpp:263-264
		return 1;
	}
	return 0;
}
