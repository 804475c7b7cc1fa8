// Micro-benchmark: stage 1 of the two-stage closest-hit scan (the slab test of DESIGN.md section 4.1: 9 multiply-adds + |gm|-|t| > Dq per
// (ray, triangle)) on the FP32 matrix pipe instead of the VALU.
//
// v_mfma_f32_4x4x1_16B_f32 computes, for 16 blocks of 4 lanes, D[i][j] = A[i]*B[j] + C[i][j] (K = 1: one fused
// multiply-add per output, no K padding).  With cbsz = 4 the A operand of block `abid` is broadcast to all 16
// blocks, so:   A = one filter coefficient of triangles 4*abid .. 4*abid+3 (lane l of the A register holds triangle l
// of a 64-triangle batch: every lane read its OWN record from LDS, 3 ds_read_b128 per 64 triangles instead of 192),
//               B = the lane's own ray component (ray per lane, as in the production kernel),
//               D register i of lane l = coefficient(triangle 4*abid+i) * ray(l) + C   -- ray per lane, 4 triangles.
// Nine such instructions per (4 triangles x 64 rays) reproduce the VALU's fmaf chains bit for bit (the guide: f32 MFMA is
// a k-ordered fmaf chain), so the survivors are the same set and the renderer's output cannot change.
//
// Modes: 0 = VALU filter as in production (broadcast LDS reads, 4 triangles x 2 rays per group)
//        1 = all nine multiply-adds of every pair on the matrix pipe, compare tree on the VALU
//        2 = mixed: of each 64-triangle batch, blocks [0, SPLIT) on the matrix pipe, the rest on the VALU
// Every mode must report the same survivor count and checksum.
//
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -o build/mfma_filter_bench tools/mfma_filter_bench.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 256, kTileQ = kTile * 3;

struct Args {
	const float4* filt; const float* rays; uint32_t n_rays, n_tris; float rv;
	unsigned long long* count; unsigned long long* sum;
};

__device__ __forceinline__ bool slab_survives(const float4 q0, const float4 q1, const float hz, float Px, float Py, float Pz, float dx, float dy, float dz, float dq) {
	float gm = q0.x * Px;
	gm = __builtin_fmaf(q0.y, Py, gm);
	gm = __builtin_fmaf(q0.z, Pz, gm);
	gm = __builtin_fmaf(-dx, q0.w, gm);
	gm = __builtin_fmaf(-dy, q1.x, gm);
	gm = __builtin_fmaf(-dz, q1.y, gm);
	float t = dx * q1.z;
	t = __builtin_fmaf(dy, q1.w, t);
	t = __builtin_fmaf(dz, hz, t);
	return !(fabsf(gm) - fabsf(t) > dq);
}

template <int B>
__device__ __forceinline__ void mfma_block(const float (&a)[9], const float (&P)[2][3], const float (&D)[2][3], const float (&ND)[2][3],
                                           const float (&Dq)[2], uint32_t base, uint32_t& cnt, unsigned long long& sum) {
	const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
	f32x4 gm[2], t[2];
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		f32x4 g = __builtin_amdgcn_mfma_f32_4x4x1f32(a[0], P[r][0], z, 4, B, 0);
		g = __builtin_amdgcn_mfma_f32_4x4x1f32(a[1], P[r][1], g, 4, B, 0);
		g = __builtin_amdgcn_mfma_f32_4x4x1f32(a[2], P[r][2], g, 4, B, 0);
		g = __builtin_amdgcn_mfma_f32_4x4x1f32(a[3], ND[r][0], g, 4, B, 0);
		g = __builtin_amdgcn_mfma_f32_4x4x1f32(a[4], ND[r][1], g, 4, B, 0);
		g = __builtin_amdgcn_mfma_f32_4x4x1f32(a[5], ND[r][2], g, 4, B, 0);
		f32x4 tt = __builtin_amdgcn_mfma_f32_4x4x1f32(a[6], D[r][0], z, 4, B, 0);
		tt = __builtin_amdgcn_mfma_f32_4x4x1f32(a[7], D[r][1], tt, 4, B, 0);
		tt = __builtin_amdgcn_mfma_f32_4x4x1f32(a[8], D[r][2], tt, 4, B, 0);
		gm[r] = g; t[r] = tt;
	}
	// reject <=> |gm| - |t| > Dq.  All inputs are finite here (non-finite rays get Dq = inf, non-finite records are replaced
	// at repack), so min() over the four triangles keeps the NaN-safe form:  any survivor <=> !(min_i x_i > Dq)
	float x[2][4];
	bool any = false;
#pragma unroll
	for (int r = 0; r < 2; ++r) {
#pragma unroll
		for (int i = 0; i < 4; ++i) x[r][i] = fabsf(gm[r][i]) - fabsf(t[r][i]);
		const float m = fminf(__builtin_fminf(x[r][0], x[r][1]), __builtin_fminf(x[r][2], x[r][3]));
		any |= !(m > Dq[r]);
	}
	if (any) {
#pragma unroll
		for (int i = 0; i < 4; ++i)
#pragma unroll
			for (int r = 0; r < 2; ++r)
				if (!(x[r][i] > Dq[r])) { ++cnt; sum += (unsigned long long)(base + 4 * B + i) * (r + 1); }
	}
}

template <int B0, int B1>
struct MfmaBlocks {
	static __device__ __forceinline__ void run(const float (&a)[9], const float (&P)[2][3], const float (&D)[2][3], const float (&ND)[2][3],
	                                           const float (&Dq)[2], uint32_t base, uint32_t& cnt, unsigned long long& sum) {
		mfma_block<B0>(a, P, D, ND, Dq, base, cnt, sum);
		MfmaBlocks<B0 + 1, B1>::run(a, P, D, ND, Dq, base, cnt, sum);
	}
};
template <int B1>
struct MfmaBlocks<B1, B1> {
	static __device__ __forceinline__ void run(const float (&)[9], const float (&)[2][3], const float (&)[2][3], const float (&)[2][3],
	                                           const float (&)[2], uint32_t, uint32_t&, unsigned long long&) {}
};

__device__ __forceinline__ void valu_groups(const float4* cur, uint32_t q0, uint32_t q1, uint32_t tri_base, const float (&P)[2][3], const float (&D)[2][3],
                                            const float (&Dq)[2], uint32_t& cnt, unsigned long long& sum) {
	for (uint32_t q = q0; q < q1; q += 12u) {
		float4 a0[4], a1[4]; float a2[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) { a0[u] = cur[q + 3 * u]; a1[u] = cur[q + 3 * u + 1]; a2[u] = cur[q + 3 * u + 2].x; }
		bool sv[4][2]; bool any = false;
#pragma unroll
		for (int u = 0; u < 4; ++u)
#pragma unroll
			for (int r = 0; r < 2; ++r) {
				sv[u][r] = slab_survives(a0[u], a1[u], a2[u], P[r][0], P[r][1], P[r][2], D[r][0], D[r][1], D[r][2], Dq[r]);
				any |= sv[u][r];
			}
		if (any) {
			const uint32_t j0 = q / 3u;
#pragma unroll
			for (int u = 0; u < 4; ++u)
#pragma unroll
				for (int r = 0; r < 2; ++r) if (sv[u][r]) { ++cnt; sum += (unsigned long long)(tri_base + j0 + u) * (r + 1); }
		}
	}
}


// ---- "cylinder" stage 1: |t| = |dir.h| replaced by its upper bound |h|*|dir| (H per triangle, D per ray):
//   reject  <=>  |gm| - H*D > Dq        (6 multiply-adds for gm, one fma for x, min-tree + one compare per 4 triangles)
// Every pair this rejects the slab test rejects too (H*D >= |t|), so conservativeness is inherited.
// record: 2 x float4:  q0 = w.x w.y w.z Mc.x   q1 = Mc.y Mc.z H _
struct CylArgs { const float4* rec; };

__device__ __forceinline__ float cyl_x(const float4 q0, const float4 q1, float Px, float Py, float Pz, float ndx, float ndy, float ndz, float D) {
	float gm = q0.x * Px;
	gm = __builtin_fmaf(q0.y, Py, gm);
	gm = __builtin_fmaf(q0.z, Pz, gm);
	gm = __builtin_fmaf(ndx, q0.w, gm);
	gm = __builtin_fmaf(ndy, q1.x, gm);
	gm = __builtin_fmaf(ndz, q1.y, gm);
	return __builtin_fmaf(-q1.z, D, fabsf(gm));
}
// axis-normalised form: the dominant component of w is exactly 1, so its product is the chain's start value
//   q0 = w_b w_c Mc.x Mc.y   q1 = Mc.z H _ _     (Pa, Pb, Pc) = P permuted so that a is the dominant axis
__device__ __forceinline__ float cyl5_x(const float4 q0, const float4 q1, float Pa, float Pb, float Pc, float ndx, float ndy, float ndz, float D) {
	float gm = __builtin_fmaf(q0.x, Pb, Pa);
	gm = __builtin_fmaf(q0.y, Pc, gm);
	gm = __builtin_fmaf(ndx, q0.z, gm);
	gm = __builtin_fmaf(ndy, q0.w, gm);
	gm = __builtin_fmaf(ndz, q1.x, gm);
	return __builtin_fmaf(-q1.y, D, fabsf(gm));
}

template <int FORM>   // 6 = cyl, 5 = axis-normalised cyl (single class in this benchmark: timing only)
__device__ __forceinline__ void cyl_groups(const float4* cur, uint32_t q0i, uint32_t q1i, uint32_t tri_base, const float (&P)[2][3], const float (&ND)[2][3],
                                           const float (&Dn)[2], const float (&Dq)[2], uint32_t& cnt, unsigned long long& sum) {
	for (uint32_t q = q0i; q < q1i; q += 8u) {
		float4 a0[4], a1[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) { a0[u] = cur[q + 2 * u]; a1[u] = cur[q + 2 * u + 1]; }
		float x[4][2];
		bool any = false;
#pragma unroll
		for (int r = 0; r < 2; ++r) {
#pragma unroll
			for (int u = 0; u < 4; ++u)
				x[u][r] = FORM == 6 ? cyl_x(a0[u], a1[u], P[r][0], P[r][1], P[r][2], ND[r][0], ND[r][1], ND[r][2], Dn[r])
				                    : cyl5_x(a0[u], a1[u], P[r][0], P[r][1], P[r][2], ND[r][0], ND[r][1], ND[r][2], Dn[r]);
			const float m = __builtin_fminf(__builtin_fminf(x[0][r], x[1][r]), __builtin_fminf(x[2][r], x[3][r]));
			any |= !(m > Dq[r]);
		}
		if (any) {
			const uint32_t j0 = q / 2u;
#pragma unroll
			for (int u = 0; u < 4; ++u)
#pragma unroll
				for (int r = 0; r < 2; ++r) if (!(x[u][r] > Dq[r])) { ++cnt; sum += (unsigned long long)(tri_base + j0 + u) * (r + 1); }
		}
	}
}

template <int FORM>
__global__ void __launch_bounds__(256, 4) k_cyl(const Args a, const float4* rec) {
	__shared__ float4 sm[2 * 512];      // 256 triangles x 32 B, double-buffered
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t k0 = blockIdx.x * 512u + tid;
	float P[2][3], ND[2][3], Dq[2], Dn[2];
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const uint32_t k = k0 + r * 256u;
		const float* p = a.rays + (size_t)(k < a.n_rays ? k : a.n_rays - 1) * 6;
		const float ox = p[0], oy = p[1], oz = p[2], dx = p[3], dy = p[4], dz = p[5];
		ND[r][0] = -dx; ND[r][1] = -dy; ND[r][2] = -dz;
		P[r][0] = oy * dz - oz * dy; P[r][1] = oz * dx - ox * dz; P[r][2] = ox * dy - oy * dx;
		const float dn = fabsf(dx) + fabsf(dy) + fabsf(dz), on = fabsf(ox) + fabsf(oy) + fabsf(oz);
		const float mag = dn * (on + 2.0f * a.rv);
		Dq[r] = k < a.n_rays ? (mag < 1e37f ? 0x1p-16f * 1.01f * mag : __builtin_inff()) : -1.0f;
		Dn[r] = __builtin_sqrtf(dx * dx + dy * dy + dz * dz) * (1.0f + 0x1p-21f);
	}
	uint32_t cnt = 0; unsigned long long sum = 0;
	const uint32_t ntiles = (a.n_tris + kTile - 1) / kTile;
	float4 p0 = rec[tid], p1 = rec[256 + tid];
	sm[tid] = p0; sm[256 + tid] = p1;
	__syncthreads();
	for (uint32_t t = 0; t < ntiles; ++t) {
		const float4* cur = sm + (t & 1u) * 512;
		const bool more = t + 1 < ntiles;
		const float4* nsrc = rec + (size_t)(more ? t + 1 : t) * 512;
		p0 = nsrc[tid]; p1 = nsrc[256 + tid];
		cyl_groups<FORM>(cur, 0, 512, t * kTile, P, ND, Dn, Dq, cnt, sum);
		float4* nxt = sm + ((t + 1) & 1u) * 512;
		nxt[tid] = p0; nxt[256 + tid] = p1;
		__syncthreads();
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) { cnt += __shfl_down(cnt, off, 64); sum += __shfl_down(sum, off, 64); }
	if (lane == 0) { atomicAdd(a.count, (unsigned long long)cnt); atomicAdd(a.sum, sum); }
}

// slab filter with the records read through the scalar cache (wave-uniform address -> s_load, SGPR operands): no LDS, no barriers
__global__ void __launch_bounds__(256, 4) k_sload(const Args a) {
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t k0 = blockIdx.x * 512u + tid;
	float P[2][3], D[2][3], Dq[2];
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const uint32_t k = k0 + r * 256u;
		const float* p = a.rays + (size_t)(k < a.n_rays ? k : a.n_rays - 1) * 6;
		const float ox = p[0], oy = p[1], oz = p[2];
		D[r][0] = p[3]; D[r][1] = p[4]; D[r][2] = p[5];
		P[r][0] = oy * D[r][2] - oz * D[r][1]; P[r][1] = oz * D[r][0] - ox * D[r][2]; P[r][2] = ox * D[r][1] - oy * D[r][0];
		const float dn = fabsf(D[r][0]) + fabsf(D[r][1]) + fabsf(D[r][2]), on = fabsf(ox) + fabsf(oy) + fabsf(oz);
		const float mag = dn * (on + 2.0f * a.rv);
		Dq[r] = k < a.n_rays ? (mag < 1e37f ? 0x1p-16f * 1.01f * mag : __builtin_inff()) : -1.0f;
	}
	uint32_t cnt = 0; unsigned long long sum = 0;
	const uint32_t n4 = (a.n_tris + 3u) & ~3u;
	valu_groups(a.filt, 0, n4 * 3u, 0, P, D, Dq, cnt, sum);
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) { cnt += __shfl_down(cnt, off, 64); sum += __shfl_down(sum, off, 64); }
	if (lane == 0) { atomicAdd(a.count, (unsigned long long)cnt); atomicAdd(a.sum, sum); }
}

template <int MODE, int SPLIT>
__global__ void __launch_bounds__(256, 4) k_bench(const Args a) {
	__shared__ float4 sm[2 * kTileQ];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t k0 = blockIdx.x * 512u + tid;
	float P[2][3], D[2][3], ND[2][3], Dq[2];
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const uint32_t k = k0 + r * 256u;
		const float* p = a.rays + (size_t)(k < a.n_rays ? k : a.n_rays - 1) * 6;
		const float ox = p[0], oy = p[1], oz = p[2];
		D[r][0] = p[3]; D[r][1] = p[4]; D[r][2] = p[5];
		ND[r][0] = -D[r][0]; ND[r][1] = -D[r][1]; ND[r][2] = -D[r][2];
		P[r][0] = oy * D[r][2] - oz * D[r][1]; P[r][1] = oz * D[r][0] - ox * D[r][2]; P[r][2] = ox * D[r][1] - oy * D[r][0];
		const float dn = fabsf(D[r][0]) + fabsf(D[r][1]) + fabsf(D[r][2]), on = fabsf(ox) + fabsf(oy) + fabsf(oz);
		const float mag = dn * (on + 2.0f * a.rv);
		Dq[r] = k < a.n_rays ? (mag < 1e37f ? 0x1p-16f * 1.01f * mag : __builtin_inff()) : -1.0f;
	}
	uint32_t cnt = 0; unsigned long long sum = 0;
	const uint32_t ntiles = (a.n_tris + kTile - 1) / kTile;
	float4 p0 = a.filt[tid], p1 = a.filt[256 + tid], p2 = a.filt[512 + tid];
	sm[tid] = p0; sm[256 + tid] = p1; sm[512 + tid] = p2;
	__syncthreads();
	for (uint32_t t = 0; t < ntiles; ++t) {
		const float4* cur = sm + (t & 1u) * kTileQ;
		const bool more = t + 1 < ntiles;
		const float4* nsrc = a.filt + (size_t)(more ? t + 1 : t) * kTileQ;
		p0 = nsrc[tid]; p1 = nsrc[256 + tid]; p2 = nsrc[512 + tid];
		if (MODE == 0) {
			valu_groups(cur, 0, kTileQ, t * kTile, P, D, Dq, cnt, sum);
		} else {
#pragma unroll 1
			for (uint32_t b = 0; b < 4; ++b) {     // 64-triangle batches: every lane reads its own record
				const float4 r0 = cur[(b * 64u + lane) * 3u + 0], r1 = cur[(b * 64u + lane) * 3u + 1], r2 = cur[(b * 64u + lane) * 3u + 2];
				const float av[9] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x };
				MfmaBlocks<0, SPLIT>::run(av, P, D, ND, Dq, t * kTile + b * 64u, cnt, sum);
				if (SPLIT < 16) valu_groups(cur, (b * 64u + 4u * SPLIT) * 3u, (b * 64u + 64u) * 3u, t * kTile, P, D, Dq, cnt, sum);
			}
		}
		float4* nxt = sm + ((t + 1) & 1u) * kTileQ;
		nxt[tid] = p0; nxt[256 + tid] = p1; nxt[512 + tid] = p2;
		__syncthreads();
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) { cnt += __shfl_down(cnt, off, 64); sum += __shfl_down(sum, off, 64); }
	if (lane == 0) { atomicAdd(a.count, (unsigned long long)cnt); atomicAdd(a.sum, sum); }
}

static uint32_t rng_state = 12345u;
static float frand() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.0f / 16777216.0f); }

int main(int argc, char** argv) {
	const uint32_t n_tris = argc > 1 ? (uint32_t)atoi(argv[1]) : 10000u;
	const uint32_t n_rays = argc > 2 ? (uint32_t)atoi(argv[2]) : (1u << 22);
	const uint32_t n_pad = (n_tris + kTile - 1) / kTile * kTile;
	// clutter like scene.closed_room: small triangles (+-0.025) in a 3 x 1.7 x 2.5 box, plus 12 room-sized ones
	std::vector<float> filt((size_t)n_pad * 12, 0.0f), cyl((size_t)n_pad * 8, 0.0f), cyl5((size_t)n_pad * 8, 0.0f);
	float rv = 0.0f;
	for (uint32_t i = 0; i < n_pad; ++i) {
		float* f = &filt[(size_t)i * 12];
		if (i >= n_tris) { f[3] = f[4] = f[5] = 1e30f; cyl[(size_t)i * 8 + 6] = -1e30f; cyl5[(size_t)i * 8 + 5] = -1e30f; continue; }
		double v[3][3];
		if (i < 12) { for (int k = 0; k < 3; ++k) { v[k][0] = (frand() < 0.5f ? -4.0 : 4.0); v[k][1] = (frand() < 0.5f ? -1.5 : 2.5); v[k][2] = (frand() < 0.5f ? -4.0 : 4.0); } }
		else {
			const double c[3] = { -1.5 + 3.0 * frand(), -1.0 + 1.7 * frand(), -0.5 + 2.5 * frand() };
			for (int k = 0; k < 3; ++k) for (int x = 0; x < 3; ++x) v[k][x] = (double)(float)(c[x] + 0.025 * (2.0 * frand() - 1.0));
		}
		for (int k = 0; k < 3; ++k) rv = fmaxf(rv, (float)(fabs(v[k][0]) + fabs(v[k][1]) + fabs(v[k][2])));
		double e1[3], e2[3], c3[3];
		for (int x = 0; x < 3; ++x) { e1[x] = (float)(v[1][x] - v[0][x]); e2[x] = (float)(v[2][x] - v[0][x]); c3[x] = e2[x] - e1[x]; }
		const double l1 = e1[0]*e1[0]+e1[1]*e1[1]+e1[2]*e1[2], l2 = e2[0]*e2[0]+e2[1]*e2[1]+e2[2]*e2[2], lc = c3[0]*c3[0]+c3[1]*c3[1]+c3[2]*c3[2];
		const double *w3, *q0, *q1; double len2;
		if (l2 >= l1 && l2 >= lc) { w3 = e2; q0 = v[0]; q1 = v[1]; len2 = l2; } else if (l1 >= lc) { w3 = e1; q0 = v[0]; q1 = v[2]; len2 = l1; } else { w3 = c3; q0 = v[1]; q1 = v[0]; len2 = lc; }
		const double len = sqrt(len2);
		if (!(len > 0)) continue;
		const double w[3] = { (float)(w3[0] / len), (float)(w3[1] / len), (float)(w3[2] / len) };
		const double pc[3] = { 0.5 * (q0[0] + q1[0]), 0.5 * (q0[1] + q1[1]), 0.5 * (q0[2] + q1[2]) }, ph[3] = { 0.5 * (q1[0] - q0[0]), 0.5 * (q1[1] - q0[1]), 0.5 * (q1[2] - q0[2]) };
		f[0] = (float)w[0]; f[1] = (float)w[1]; f[2] = (float)w[2];
		f[3] = (float)(w[1] * pc[2] - w[2] * pc[1]); f[4] = (float)(w[2] * pc[0] - w[0] * pc[2]); f[5] = (float)(w[0] * pc[1] - w[1] * pc[0]);
		f[6] = (float)(w[1] * ph[2] - w[2] * ph[1]); f[7] = (float)(w[2] * ph[0] - w[0] * ph[2]); f[8] = (float)(w[0] * ph[1] - w[1] * ph[0]);
		{
			float* c = &cyl[(size_t)i * 8];
			for (int x = 0; x < 6; ++x) c[x] = f[x];
			const double H = sqrt((double)f[6] * f[6] + (double)f[7] * f[7] + (double)f[8] * f[8]);
			c[6] = (float)(H * (1.0 + 0x1p-21));
			// axis-normalised (timing only here: every record is written as if x were dominant, scaled by 1/|w| max)
			const double s = 1.0 / fmax(fabs(w[0]), fmax(fabs(w[1]), fabs(w[2])));
			float* c5 = &cyl5[(size_t)i * 8];
			c5[0] = (float)(w[1] * s); c5[1] = (float)(w[2] * s); c5[2] = (float)(f[3] * s); c5[3] = (float)(f[4] * s); c5[4] = (float)(f[5] * s); c5[5] = (float)(H * s * (1.0 + 0x1p-21));
		}
	}
	std::vector<float> rays((size_t)n_rays * 6);
	for (uint32_t i = 0; i < n_rays; ++i) {
		float* r = &rays[(size_t)i * 6];
		r[0] = -3.5f + 7.0f * frand(); r[1] = -1.2f + 3.4f * frand(); r[2] = -3.5f + 7.0f * frand();
		float d[3], l;
		do { for (int x = 0; x < 3; ++x) d[x] = 2.0f * frand() - 1.0f; l = sqrtf(d[0]*d[0]+d[1]*d[1]+d[2]*d[2]); } while (l < 0.1f || l > 1.0f);
		r[3] = d[0] / l; r[4] = d[1] / l; r[5] = d[2] / l;
	}
	float4* d_filt; float* d_rays; unsigned long long* d_cnt;
	CHECK(hipMalloc(&d_filt, filt.size() * 4)); CHECK(hipMalloc(&d_rays, rays.size() * 4)); CHECK(hipMalloc(&d_cnt, 16));
	CHECK(hipMemcpy(d_filt, filt.data(), filt.size() * 4, hipMemcpyHostToDevice));
	CHECK(hipMemcpy(d_rays, rays.data(), rays.size() * 4, hipMemcpyHostToDevice));
	float4 *d_cyl, *d_cyl5;
	CHECK(hipMalloc(&d_cyl, cyl.size() * 4)); CHECK(hipMalloc(&d_cyl5, cyl5.size() * 4));
	CHECK(hipMemcpy(d_cyl, cyl.data(), cyl.size() * 4, hipMemcpyHostToDevice)); CHECK(hipMemcpy(d_cyl5, cyl5.data(), cyl5.size() * 4, hipMemcpyHostToDevice));
	Args a{ d_filt, d_rays, n_rays, n_tris, rv, d_cnt, d_cnt + 1 };
	const dim3 grid((n_rays + 511) / 512), block(256);
	hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
	const double pairs = (double)n_rays * n_tris;
	unsigned long long ref[2] = {0, 0};
	auto run_l = [&](const char* name, auto launch) {
		float best = 1e30f; unsigned long long res[2];
		for (int it = 0; it < 4; ++it) {
			CHECK(hipMemset(d_cnt, 0, 16));
			CHECK(hipEventRecord(e0));
			launch();
			CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
			float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (it && ms < best) best = ms;
		}
		CHECK(hipGetLastError());
		CHECK(hipMemcpy(res, d_cnt, 16, hipMemcpyDeviceToHost));
		if (!ref[0]) { ref[0] = res[0]; ref[1] = res[1]; }
		printf("%-34s %8.3f ms  %6.3f T pairs/s  survivors %llu (%.4f %%) checksum %llu %s\n", name, best, pairs / best * 1e-9, res[0], 100.0 * res[0] / pairs, res[1],
		       (res[0] == ref[0] && res[1] == ref[1]) ? "== VALU" : "MISMATCH");
		fflush(stdout);
	};
	auto run = [&](const char* name, void (*kern)(const Args)) { run_l(name, [&] { hipLaunchKernelGGL(kern, grid, block, 0, 0, a); }); };
	printf("stage-1 micro-benchmark: %u triangles x %u rays (2 per lane), no queue, no exact stage\n", n_tris, n_rays);
	run("VALU (production form)", k_bench<0, 0>);
	run("MFMA 4x4x1_16B, all 16 blocks", k_bench<1, 16>);
	run("mixed: 14 blocks MFMA + 2 VALU", k_bench<2, 14>);
	run("mixed: 12 blocks MFMA + 4 VALU", k_bench<2, 12>);
	run("mixed: 10 blocks MFMA + 6 VALU", k_bench<2, 10>);
	run("mixed:  8 blocks MFMA + 8 VALU", k_bench<2, 8>);
	run("VALU slab, records via s_load (no LDS)", k_sload);
	run_l("cylinder test, 6 fma (more survivors)", [&] { hipLaunchKernelGGL(k_cyl<6>, grid, block, 0, 0, a, (const float4*)d_cyl); });
	run_l("cylinder, axis-normalised 5 fma (timing)", [&] { hipLaunchKernelGGL(k_cyl<5>, grid, block, 0, 0, a, (const float4*)d_cyl5); });
	return 0;
}
