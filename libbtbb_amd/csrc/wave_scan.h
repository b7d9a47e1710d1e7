// wave_scan.h -- prefix sums over the lanes of a wave and the threads of a workgroup (packet.hip, sort.hip, survey.hip).
#pragma once
#include <stdint.h>

// inclusive prefix sum over the lanes of a wave (WIDTH 64), or over its first WIDTH lanes; lane = the caller's lane number
template <int WIDTH>
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < WIDTH; d <<= 1) {
		const uint32_t up = __shfl_up(v, d);
		if (lane >= (uint32_t)d)
			v += up;
	}
	return v;
}

// exclusive prefix sum over the 64 WAVES threads of a workgroup, total = the sum of all; lds: WAVES words; ends with a barrier
template <uint32_t WAVES>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *lds, uint32_t &total)
{
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t inc = wave_inclusive_scan<64>(v, lane);
	if (lane == 63)
		lds[wave] = inc;
	__syncthreads();
	uint32_t before = 0, sum = 0;
	for (uint32_t w = 0; w < WAVES; w++) {
		const uint32_t t = lds[w];
		if (w < wave)
			before += t;
		sum += t;
	}
	total = sum;
	__syncthreads();
	return before + inc - v;
}
