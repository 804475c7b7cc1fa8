// Adaptive sampling (include/spath_hip.h: sphip_accum_begin_adaptive): after each step of a progressive
// accumulation, the convergence rule stops the pixels whose estimate has settled, the survivors are compacted into a dense
// list in ascending pixel order for the next step's launch, and the whole frame is resolved from the per-pixel sums and counts.
//
// Compaction: k_adapt_decide applies the rule to launch ray k (= local pixel list[k]) and counts the survivors of its block
// (64-bit ballot + popcount per wave, wave totals in LDS); k_adapt_scan turns the block totals into exclusive offsets in one
// workgroup; k_adapt_scatter writes survivor k to offset(block) + survivors before it in its block.  No atomics: the new list
// (and the gathered rays) depend on nothing but the decisions.
#pragma once

#include "sp_kernels.h"

namespace sp {

struct AdaptRule {
	double t, floor;           // relative error, the mean below which the error is measured absolutely
	uint32_t min_samples;      // >= 2
	uint32_t n_step;           // samples the step added to every active pixel
};

// the rule of include/spath_hip.h, in double, in the stated order (the build has -ffp-contract=off: nothing is fused)
SP_DEV bool adapt_converged(const AdaptRule& R, double s1, double s2, uint32_t count) {
	const double n = (double)count;
	const double m = s1 / n;
	const double v = (s2 - s1 * m) / (n - 1.0);
	const double r = m > R.floor ? m : R.floor;
	const double d = R.t * r;
	return v / n <= d * d;
}

// survivors before this lane in its workgroup, and (lane 0 of wave 0) the workgroup's total; must be called by all 256 threads
SP_DEV uint32_t block_rank(bool keep, uint32_t* total) {
	__shared__ uint32_t wcnt[4];
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	const unsigned long long m = __ballot(keep);
	if (lane == 0) wcnt[wv] = (uint32_t)__popcll(m);
	__syncthreads();
	uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
	for (uint32_t w = 0; w < wv; ++w) before += wcnt[w];
	if (threadIdx.x == 0) *total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
	return before;
}

// rule + counts for the n_act pixels of the step's launch; keep[k] = pixel list[k] stays active; block_tot[b] = survivors of block b
__global__ void __launch_bounds__(256) k_adapt_decide(const uint32_t* __restrict__ list, uint32_t n_act, uint32_t* __restrict__ counts,
                                                      const double* __restrict__ s12, const AdaptRule R, uint8_t* __restrict__ keep,
                                                      uint32_t* __restrict__ block_tot) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	bool kp = false;
	if (k < n_act) {
		const uint32_t p = list[k];
		const uint32_t c = counts[p] + R.n_step;
		counts[p] = c;
		kp = !(c >= R.min_samples && adapt_converged(R, s12[(size_t)p * 2], s12[(size_t)p * 2 + 1], c));
		keep[k] = kp ? 1 : 0;
	}
	uint32_t tot = 0;
	(void)block_rank(kp, &tot);
	if (threadIdx.x == 0) block_tot[blockIdx.x] = tot;
}

// exclusive scan of block_tot[0, n_blocks) in place, in one workgroup of 1024 threads; *n_active = the sum
__global__ void __launch_bounds__(1024) k_adapt_scan(uint32_t* __restrict__ block_tot, uint32_t n_blocks, uint32_t* __restrict__ n_active) {
	__shared__ uint32_t part[1024];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_blocks; base += 1024u) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n_blocks ? block_tot[i] : 0u;
		part[threadIdx.x] = v;
		__syncthreads();
		for (uint32_t off = 1; off < 1024u; off <<= 1) {            // Hillis-Steele inclusive scan
			const uint32_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
			__syncthreads();
			part[threadIdx.x] += add;
			__syncthreads();
		}
		if (i < n_blocks) block_tot[i] = carry + part[threadIdx.x] - v;
		carry += part[1023];
		__syncthreads();                                          // part is rewritten by the next round
	}
	if (threadIdx.x == 0) *n_active = carry;
}

// survivor k -> new_list[block_off[b] + rank], with its ray gathered from the accumulation's full ray buffer
__global__ void __launch_bounds__(256) k_adapt_scatter(const uint32_t* __restrict__ list, uint32_t n_act, const uint8_t* __restrict__ keep,
                                                       const uint32_t* __restrict__ block_off, const float* __restrict__ rays,
                                                       uint32_t* __restrict__ new_list, float* __restrict__ new_rays) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool kp = k < n_act && keep[k];
	uint32_t tot;
	const uint32_t o = block_off[blockIdx.x] + block_rank(kp, &tot);
	if (!kp) return;
	const uint32_t p = list[k];
	new_list[o] = p;
#pragma unroll
	for (int c = 0; c < 6; ++c) new_rays[(size_t)o * 6 + c] = rays[(size_t)p * 6 + c];
}

// every pixel of the shard from its running sum and count: the epilogue of the path kernels (cpu_renderer.cpp:77-78) with
// inv_n = float(1.0 / count), as the host forms it for a plain launch
__global__ void __launch_bounds__(256) k_adapt_resolve(const float* __restrict__ sum, const uint32_t* __restrict__ counts, uint32_t n,
                                                       uint32_t* __restrict__ out_rgba, float* __restrict__ out_mean) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint32_t c = counts[p];
	const float inv_n = (float)(1.0 / (double)(c ? c : 1u));
	const f3 av = scale3(mk3(sum[(size_t)p * 3 + 0], sum[(size_t)p * 3 + 1], sum[(size_t)p * 3 + 2]), inv_n);
	out_rgba[p] = vec3_rgba(mk3(clamp01(av.x), clamp01(av.y), clamp01(av.z)));
	if (out_mean) {
		out_mean[(size_t)p * 3 + 0] = av.x;
		out_mean[(size_t)p * 3 + 1] = av.y;
		out_mean[(size_t)p * 3 + 2] = av.z;
	}
}

// first list of an accumulation: every local pixel, in order
__global__ void __launch_bounds__(256) k_adapt_iota(uint32_t* __restrict__ list, uint32_t n) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p < n) list[p] = p;
}

} // namespace sp
