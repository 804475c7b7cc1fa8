// The per-triangle scene tables of libspath_hip.so as data, and the checks of what a host-pointer setter is handed: rows of a table,
// texels of a context-level image (the environment map, the atlas, the normal map).  No HIP, like sp_host_plan.h: a host compiler builds this header
// alone, and tests/test_host_tables.py holds every rule and every message to literals.  spath_hip.hip is its one user; its generic
// setters (set_table, set_table_device) walk kTriTables, so a new table is one row here, where it lives in a context (kTableSlots
// there) and a pair of one-line entry points.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>

namespace sp_host {

struct TriTable {
	const char* name;                       // for tools and tests
	const char* setter;                     // the host-pointer entry point as the messages name it; the device form appends "_device"
	int floats;                             // per triangle (at most 9: bad_row_message)
	bool (*row_ok)(const float* row);
	const char* bad_row;                    // the message of a refused row, a printf format: %zu (the triangle), then `floats` times %g
	size_t max_tris;                        // the scene must have fewer triangles than this (0: any scene) ...
	const char* too_large;                  // ... or the setter says this, a printf format: %zu (the scene's triangles)
	bool zero_rows;                         // setting it allocates the zeros that stand in for a table whose flag is off (ensure_zero_rows)
};

inline bool finite_row(const float* q, int n) {
	for (int k = 0; k < n; ++k) if (!std::isfinite(q[k])) return false;
	return true;
}
inline bool finite_nonneg_row(const float* q, int n) {
	for (int k = 0; k < n; ++k) if (!std::isfinite(q[k]) || !(q[k] >= 0.0f)) return false;
	return true;
}

enum TriTableId { kTabSpecular, kTabVertexNormals, kTabDielectric, kTabRoughness, kTabUv, kTriTableCount };
// kSpecBit (2^30) and kTransBit (2^29) mark a mirror and a transmitted bounce in the path history: triangle indices must stay below them
inline constexpr TriTable kTriTables[kTriTableCount] = {
	{ "specular", "sphip_set_specular", 4, [](const float* q) { return finite_nonneg_row(q, 4) && q[3] <= 1.0f; },
	  "specular table: triangle %zu has {ks %g %g %g, p %g} (every value finite, ks >= 0, 0 <= p <= 1)",
	  (size_t)1 << 30, "a specular table needs a scene of fewer than 2^30 triangles (this one has %zu)", false },
	{ "vertex_normals", "sphip_set_vertex_normals", 9, [](const float* q) { return finite_row(q, 9); },
	  "vertex normals: triangle %zu has {%g %g %g, %g %g %g, %g %g %g} (every value finite)", 0, nullptr, false },
	{ "dielectric", "sphip_set_dielectric", 4, [](const float* q) { return finite_nonneg_row(q, 4) && (q[3] == 0.0f || q[3] >= 1.0f); },
	  "dielectric table: triangle %zu has {kt %g %g %g, ior %g} (every value finite, kt >= 0, ior 0 or >= 1)",
	  (size_t)1 << 29, "a dielectric table needs a scene of fewer than 2^29 triangles (this one has %zu)", true },
	{ "roughness", "sphip_set_roughness", 1, [](const float* q) { return finite_nonneg_row(q, 1) && q[0] <= 1.0f; },
	  "roughness table: triangle %zu has alpha %g (finite, 0 <= alpha <= 1)", 0, nullptr, false },
	{ "uv", "sphip_set_uv", 6, [](const float* q) { return finite_row(q, 6); },
	  "UV table: triangle %zu has {%g %g, %g %g, %g %g} (every value finite)", 0, nullptr, false },
};

// the first triangle whose row breaks the table's rule, or n_tris
inline size_t first_bad_row(const TriTable& t, const float* rows, size_t n_tris) {
	for (size_t i = 0; i < n_tris; ++i) if (!t.row_ok(rows + i * (size_t)t.floats)) return i;
	return n_tris;
}
inline std::string bad_row_message(const TriTable& t, const float* rows, size_t tri) {
	double v[9] = {};                           // a format reads its `floats` values and leaves the rest
	for (int k = 0; k < t.floats; ++k) v[k] = (double)rows[tri * (size_t)t.floats + (size_t)k];
	char buf[512];
	snprintf(buf, sizeof buf, t.bad_row, tri, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
	return buf;
}

// the texels of an image, `count` floats {r g b} in rows of `width` texels: the first float that is negative or not finite, or count
inline size_t first_bad_texel(const float* texels, size_t count) {
	for (size_t k = 0; k < count; ++k) if (!std::isfinite(texels[k]) || !(texels[k] >= 0.0f)) return k;
	return count;
}
inline std::string bad_texel_message(const char* noun, const float* texels, size_t k, size_t width) {
	char buf[512];
	snprintf(buf, sizeof buf, "%s: texel (%zu, %zu) has component %zu = %g (every value finite and >= 0)", noun, (k / 3) % width, (k / 3) / width, k % 3,
	         (double)texels[k]);
	return buf;
}

// ... of an image whose values are signed (the normal map): the first float that is not finite, or count
inline size_t first_nonfinite_texel(const float* texels, size_t count) {
	for (size_t k = 0; k < count; ++k) if (!std::isfinite(texels[k])) return k;
	return count;
}
inline std::string nonfinite_texel_message(const char* noun, const float* texels, size_t k, size_t width) {
	char buf[512];
	snprintf(buf, sizeof buf, "%s: texel (%zu, %zu) has component %zu = %g (every value finite)", noun, (k / 3) % width, (k / 3) / width, k % 3,
	         (double)texels[k]);
	return buf;
}

} // namespace sp_host
