// Display transform (include/spath_hip.h: "display transform"): a luminance histogram for metering and the
// one pass that turns a mean image into pixels -- exposure, a tone curve, vec3::clamp, and the linear or the sRGB encoding.  A
// post-process like the denoiser: nothing here is reached by the scan or path kernels.
//
// Every operation is an f32 + - * / (IEEE division), a comparison, a select, a bit cast or an integer operation, in the order the
// header states (the build has -ffp-contract=off: nothing is fused), so that tests/display_model.py replays the output bit for bit.
#pragma once

#include "sp_kernels.h"
#include "sp_srgb_table.h"

namespace sp {

constexpr uint32_t kLumBins = 2048;        // bits(l) >> 20: the f32 exponent and the top three mantissa bits

// T[k] at index k; index 0 is never read
__constant__ uint32_t c_srgb_bits[256] = { 0u, SP_SRGB_THRESHOLD_BITS };

SP_DEV float display_lum(f3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// the bin of a pixel: 0 for !(l > 0) (zero, negative, NaN), else the top 11 bits below the sign (+inf: 2040)
SP_DEV uint32_t lum_bin(f3 c) {
	const float l = display_lum(c);
	return l > 0.0f ? (__float_as_uint(l) >> 20) : 0u;
}

// One pixel of each lane into the workgroup's LDS histogram.  A flat image puts all 64 lanes of a wave into one bin, and 64 LDS atomics on
// one address execute one after the other; so equal bins are first aggregated within the wave: the lowest pending lane's bin is
// broadcast, the lanes that hold it are counted by a ballot, one of them adds the count, and all of them are done.  After four such
// rounds (a constant image needs one, an image of a few levels a few) whatever is left is spread over many bins, where per-lane LDS
// atomics run in parallel, and goes the plain way.  Must be reached by every lane of the wave (`pending` false for a lane without a pixel).
SP_DEV void hist_add(uint32_t* s_h, uint32_t bin, bool pending) {
	const uint32_t lane = __lane_id();
	for (int r = 0; r < 4; ++r) {
		if (!__any(pending)) return;
		if (pending) {
			const uint32_t b = __builtin_amdgcn_readfirstlane(bin);
			const unsigned long long same = __ballot(bin == b);
			if (bin == b) {
				if (lane == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&s_h[b], (uint32_t)__popcll(same));
				pending = false;
			}
		}
	}
	if (pending) atomicAdd(&s_h[bin], 1u);
}

// the four pixels 4 q .. 4 q + 3 of an n-pixel f32 rgb image; vec: the image is 16-byte aligned, so a whole quad is three float4
SP_DEV void load_quad(const float* __restrict__ mean, uint32_t q, uint32_t n, bool vec, f3 (&c)[4], bool (&have)[4]) {
	const size_t p0 = (size_t)q * 4;
	if (vec && p0 + 4 <= (size_t)n) {
		const float4* m4 = (const float4*)(mean + p0 * 3);
		const float4 a = m4[0], b = m4[1], d = m4[2];
		c[0] = mk3(a.x, a.y, a.z); c[1] = mk3(a.w, b.x, b.y); c[2] = mk3(b.z, b.w, d.x); c[3] = mk3(d.y, d.z, d.w);
		have[0] = have[1] = have[2] = have[3] = true;
		return;
	}
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		have[k] = p0 + (size_t)k < (size_t)n;
		c[k] = mk3(0.0f, 0.0f, 0.0f);
		if (have[k]) c[k] = mk3(mean[(p0 + k) * 3 + 0], mean[(p0 + k) * 3 + 1], mean[(p0 + k) * 3 + 2]);
	}
}

// 2048 u32 bins of an n-pixel mean image added to out (zeroed by the caller on the same stream).  Each workgroup keeps a histogram in LDS
// (8 KB) and flushes its non-zero bins with global atomics; integer sums, so the result does not depend on the order they land in.
// nq = quads of the image; every lane of a workgroup runs the same number of rounds (hist_add needs whole waves).
__global__ void __launch_bounds__(256) k_lum_histogram(const float* __restrict__ mean, uint32_t n, uint32_t nq, uint32_t vec, uint32_t* __restrict__ out) {
	__shared__ uint32_t s_h[kLumBins];
	for (uint32_t i = threadIdx.x; i < kLumBins; i += 256u) s_h[i] = 0u;
	__syncthreads();
	for (uint32_t base = blockIdx.x * 256u; base < nq; base += gridDim.x * 256u) {
		const uint32_t q = base + threadIdx.x;
		f3 c[4];
		bool have[4] = { false, false, false, false };
		if (q < nq) load_quad(mean, q, n, vec != 0u, c, have);
#pragma unroll
		for (int k = 0; k < 4; ++k) hist_add(s_h, have[k] ? lum_bin(c[k]) : 0u, have[k]);
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kLumBins; i += 256u) {
		const uint32_t v = s_h[i];
		if (v) atomicAdd(&out[i], v);
	}
}

struct DisplayArgs {
	const float* mean;      // n * 3 f32
	uint32_t* rgba;         // n u32
	float* rgb;             // n * 3 f32 or nullptr
	uint32_t n;
	float exposure;
	float w2;               // white * white (f32, formed by the host)
	uint32_t curve, encode;
	uint32_t vec;           // every pointer is 16-byte aligned: whole quads move as float4 / uint4
};

// Narkowicz's fit of the ACES filmic curve, per channel
SP_DEV float filmic(float x) { return (x * ((2.51f * x) + 0.03f)) / ((x * ((2.43f * x) + 0.59f)) + 0.14f); }

// exposure, curve and vec3::clamp: the display-linear triple in [0, 1] (the float output)
SP_DEV f3 display_linear(f3 c, const DisplayArgs& A) {
	f3 v = scale3(c, A.exposure);
	if (A.curve == 1u) {                       // extended Reinhard on luminance
		const float l = display_lum(v);
		if (l > 0.0f) v = scale3(v, (1.0f + l / A.w2) / (1.0f + l));
	} else if (A.curve == 2u)
		v = mk3(filmic(v.x), filmic(v.y), filmic(v.z));
	return mk3(clamp01(v.x), clamp01(v.y), clamp01(v.z));
}

// the number of k in 1 .. 255 with x >= T[k]: 8 steps over the table in LDS; every comparison with a NaN fails, so a NaN is 0
SP_DEV uint32_t srgb_code(const float* s_T, float x) {
	uint32_t lo = 0u;
#pragma unroll
	for (uint32_t step = 128u; step > 0u; step >>= 1) lo += (x >= s_T[lo + step]) ? step : 0u;
	return lo;
}

SP_DEV uint32_t display_encode(const float* s_T, f3 v, uint32_t encode) {
	return encode == 1u ? (srgb_code(s_T, v.x) | (srgb_code(s_T, v.y) << 8) | (srgb_code(s_T, v.z) << 16)) : vec3_rgba(v);
}

// mean -> RGBA8 (+ the display-linear float), four pixels per lane: 48 B in, 16 B (+ 48 B) out
__global__ void __launch_bounds__(256) k_display(const DisplayArgs A) {
	__shared__ float s_T[256];
	if (A.encode == 1u) {
		s_T[threadIdx.x] = __uint_as_float(c_srgb_bits[threadIdx.x]);
		__syncthreads();
	}
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	const size_t p0 = (size_t)q * 4;
	if (p0 >= (size_t)A.n) return;
	f3 c[4];
	bool have[4];
	load_quad(A.mean, q, A.n, A.vec != 0u, c, have);
	f3 v[4];
	uint32_t px[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		v[k] = display_linear(c[k], A);
		px[k] = display_encode(s_T, v[k], A.encode);
	}
	if (A.vec && have[3]) {
		*(uint4*)(A.rgba + p0) = make_uint4(px[0], px[1], px[2], px[3]);
		if (A.rgb) {
			float4* o4 = (float4*)(A.rgb + p0 * 3);
			o4[0] = make_float4(v[0].x, v[0].y, v[0].z, v[1].x);
			o4[1] = make_float4(v[1].y, v[1].z, v[2].x, v[2].y);
			o4[2] = make_float4(v[2].z, v[3].x, v[3].y, v[3].z);
		}
		return;
	}
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		if (!have[k]) continue;
		A.rgba[p0 + k] = px[k];
		if (A.rgb) { A.rgb[(p0 + k) * 3 + 0] = v[k].x; A.rgb[(p0 + k) * 3 + 1] = v[k].y; A.rgb[(p0 + k) * 3 + 2] = v[k].z; }
	}
}

} // namespace sp
