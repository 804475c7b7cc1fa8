// The stand-alone program of tests/test_host_plan.py and tests/test_host_tables.py: spath_amd/csrc/sp_host_plan.h and sp_host_tables.h
// under a host compiler and its sanitizers.
//   host_plan_driver plan n_rays n_samples forced pt R split scan bthreads features samp_cap work_cap free
//       prints the LaunchPlan as "name=value" words; features: bit k = member k of sp_host::Features; free: what the free-memory
//       callable reports (negative: it cannot tell); "asked" is how often it was called
//   host_plan_driver lights in out
//       in:  u64 n_tris, f64 W_env (0: no flagged table), f32 tris[n_tris * 12], f32 mats[n_tris * 6]
//       out: i64 bad_tri (-1: none), i64 bad_comp, then per table (the unflagged one, the flagged one if W_env > 0) u64 n, f64 W, the blob
//   host_plan_driver table name n_tris value...
//       the rows of the table called `name` in kTriTables (n_tris x its floats values, as strtof reads them: "nan", "-inf"): prints
//       first_bad_row (n_tris: every row passes), then on a line of its own bad_row_message for that row if there is one
//   host_plan_driver texels noun w h value...
//       an image of w x h x 3 values: prints first_bad_texel (w * h * 3: every texel passes), then bad_texel_message if there is one
#include "sp_host_plan.h"
#include "sp_host_tables.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>

using namespace sp_host;

static int plan(char** v) {
	auto u = [&](int k) { return (uint64_t)strtoull(v[k], nullptr, 10); };
	const uint32_t bits = (uint32_t)u(8);
	auto bit = [&](int k) { return ((bits >> k) & 1u) != 0; };
	const Features f{ bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8) };
	const TwoStage ts{ (int)u(4), u(5) != 0, (int)u(6) };
	const int64_t free_b = strtoll(v[11], nullptr, 10);
	int asked = 0;
	const LaunchPlan p = plan_launch(u(0), u(1), (uint32_t)u(2), u(3) != 0, ts, (uint32_t)u(7), f, u(9), u(10), [&] { ++asked; return free_b; });
	printf("chunks=%u px_blocks=%u samp_stride=%u samp_bytes=%" PRIu64 " grid=%u grid_px=%u grid_pt=%u n_work=%u n_launches=%u slot_work=%zu "
	       "slot_adp_wst=%zu slot_env_M=%zu too_large=%d asked=%d\n", p.chunks, p.px_blocks, p.samp_stride, p.samp_bytes, p.grid, p.grid_px, p.grid_pt,
	       p.n_work, p.n_launches, p.slot.work, p.slot.adp_wst, p.slot.env_M, (int)p.too_large, asked);
	return 0;
}

// the table as the device gets it, after a check that light_view finds in the blob what pack_light_table put there
static bool put_table(FILE* out, const LightTable& t) {
	const std::vector<char> blob = pack_light_table(t);
	const uint64_t n = t.cdf.size();
	const LightView w = light_view(blob.data(), n);
	for (size_t k = 0; k < n; ++k)
		if (memcmp(&w.cdf[k], &t.cdf[k], 8) || w.tri[k] != t.tri[k] || memcmp(&w.ipdf[k], &t.ipdf[k], 4)) return false;
	if (!t.tipdf.empty() && memcmp(w.tipdf, t.tipdf.data(), t.tipdf.size() * 4)) return false;
	return fwrite(&n, 8, 1, out) == 1 && fwrite(&t.W, 8, 1, out) == 1 && (blob.empty() || fwrite(blob.data(), blob.size(), 1, out) == 1);
}

static int lights(const char* in_path, const char* out_path) {
	FILE* in = fopen(in_path, "rb");
	uint64_t n = 0;
	double W_env = 0.0;
	if (!in || fread(&n, 8, 1, in) != 1 || fread(&W_env, 8, 1, in) != 1) return 2;
	std::vector<float> tris(n * 12), mats(n * 6);
	if (fread(tris.data(), 4, tris.size(), in) != tris.size() || fread(mats.data(), 4, mats.size(), in) != mats.size()) return 2;
	fclose(in);
	const LightTable t = build_light_table(tris.data(), mats.data(), n);
	FILE* out = fopen(out_path, "wb");
	if (!out) return 2;
	const int64_t bad[2] = { t.bad_tri == SIZE_MAX ? -1 : (int64_t)t.bad_tri, t.bad_comp };
	bool ok = fwrite(bad, 8, 2, out) == 2;
	if (ok && bad[0] < 0) {
		ok = put_table(out, t);
		if (ok && W_env > 0.0) ok = put_table(out, flagged_light_table(t, W_env, n));
	}
	return fclose(out) == 0 && ok ? 0 : 3;
}

static std::vector<float> values(int n, char** v) {
	std::vector<float> x((size_t)n);
	for (int k = 0; k < n; ++k) x[(size_t)k] = strtof(v[k], nullptr);
	return x;
}

static int table(int argc, char** v) {
	const size_t n_tris = (size_t)strtoull(v[1], nullptr, 10);
	for (const TriTable& t : kTriTables) {
		if (strcmp(t.name, v[0]) || (size_t)(argc - 2) != n_tris * (size_t)t.floats) continue;
		const std::vector<float> rows = values(argc - 2, v + 2);
		const size_t bad = first_bad_row(t, rows.data(), n_tris);
		printf("%zu\n", bad);
		if (bad < n_tris) printf("%s\n", bad_row_message(t, rows.data(), bad).c_str());
		return 0;
	}
	return 2;
}

static int texels(int argc, char** v) {
	const size_t w = (size_t)strtoull(v[1], nullptr, 10), h = (size_t)strtoull(v[2], nullptr, 10), count = w * h * 3;
	if ((size_t)(argc - 3) != count) return 2;
	const std::vector<float> x = values(argc - 3, v + 3);
	const size_t bad = first_bad_texel(x.data(), count);
	printf("%zu\n", bad);
	if (bad < count) printf("%s\n", bad_texel_message(v[0], x.data(), bad, w).c_str());
	return 0;
}

int main(int argc, char** argv) {
	if (argc == 14 && !strcmp(argv[1], "plan")) return plan(argv + 2);
	if (argc == 4 && !strcmp(argv[1], "lights")) return lights(argv[2], argv[3]);
	if (argc >= 4 && !strcmp(argv[1], "table")) return table(argc - 2, argv + 2);
	if (argc >= 5 && !strcmp(argv[1], "texels")) return texels(argc - 2, argv + 2);
	fprintf(stderr, "usage: host_plan_driver plan <12 numbers> | lights <in> <out> | table <name> <n_tris> <values> | texels <noun> <w> <h> <values>\n");
	return 2;
}
