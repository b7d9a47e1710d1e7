// Host check of the wide bit-sliced counters of libbtbb_amd/csrc/bitslice.h that the LE Coded PHY scan is built from: bs_add<N>
// over every pair of N-bit values (N = 1 .. 8), bs_shift_add<N> over random planes, bs_le<8> over every count and every limit,
// and le_coded_filter -- the composition -- against the plain count of equal symbol pairs over streams of several kinds and every
// limit 0 .. 63.  Built by tests/test_bitslice_coded_networks.py with the system g++; prints one line per failing case and returns
// their number (capped).
#include <stdio.h>
#include "../../libbtbb_amd/csrc/bitslice.h"

static int failures = 0;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 16);
}

// planes of the 32 values v[0..31]
static void planes_of(const uint32_t *v, int n, uint32_t *P)
{
	for (int k = 0; k < n; k++) {
		P[k] = 0;
		for (int p = 0; p < 32; p++)
			P[k] |= ((v[p] >> k) & 1u) << p;
	}
}
static uint32_t value_of(const uint32_t *P, int n, int p)
{
	uint32_t v = 0;
	for (int k = 0; k < n; k++)
		v |= ((P[k] >> p) & 1u) << k;
	return v;
}

template <int N>
static void check_add()
{
	// every pair (a, b) of N-bit values: 32 pairs per call
	const uint32_t pairs = 1u << (2 * N);
	for (uint32_t base = 0; base < pairs; base += 32) {
		uint32_t va[32], vb[32], A[N], B[N], O[N + 1];
		for (uint32_t p = 0; p < 32; p++) {
			va[p] = ((base + p) % pairs) & ((1u << N) - 1);
			vb[p] = ((base + p) % pairs) >> N;
		}
		planes_of(va, N, A);
		planes_of(vb, N, B);
		bs_add<N>(A, B, O);
		for (int p = 0; p < 32; p++)
			if (value_of(O, N + 1, p) != va[p] + vb[p] && failures++ < 20)
				printf("bs_add<%d>: %u + %u gives %u\n", N, va[p], vb[p], value_of(O, N + 1, p));
	}
	// the shifted form: lo + (hi:lo >> sh) for random planes and every shift
	for (int trial = 0; trial < 64; trial++)
		for (uint32_t sh = 1; sh < 32; sh++) {
			uint32_t lo[N], hi[N], O[N + 1];
			for (int k = 0; k < N; k++) {
				lo[k] = rnd();
				hi[k] = rnd();
			}
			bs_shift_add<N>(lo, hi, sh, O);
			for (uint32_t p = 0; p < 32; p++) {
				const uint32_t q = p + sh;
				const uint32_t other = q < 32 ? value_of(lo, N, (int)q) : value_of(hi, N, (int)(q - 32));
				if (value_of(O, N + 1, (int)p) != value_of(lo, N, (int)p) + other && failures++ < 20)
					printf("bs_shift_add<%d>: shift %u offset %u\n", N, sh, p);
			}
		}
}

static void check_le()
{
	for (uint32_t limit = 0; limit < 256; limit++)
		for (uint32_t base = 0; base < 256; base += 32) {
			uint32_t v[32], P[8], want = 0;
			for (uint32_t p = 0; p < 32; p++) {
				v[p] = base + p;
				want |= (uint32_t)(v[p] <= limit) << p;
			}
			planes_of(v, 8, P);
			if (bs_le<8>(P, limit) != want && failures++ < 20)
				printf("bs_le<8>: limit %u counts %u..\n", limit, base);
		}
}

// symbol x of the sixteen dwords
static uint32_t sym(const uint32_t *D, uint32_t x) { return (D[x >> 5] >> (x & 31)) & 1u; }

static void check_filter(const uint32_t *D, const char *what)
{
	uint32_t count[128];
	for (uint32_t o = 0; o < 128; o++) {
		count[o] = 0;
		for (uint32_t k = 0; k < 320; k++)
			if ((k & 3) < 2)
				count[o] += sym(D, o + k) == sym(D, o + k + 2);
	}
	for (uint32_t limit = 0; limit < 64; limit++) {
		uint32_t m[4];
		le_coded_filter(D, limit, m);
		for (uint32_t o = 0; o < 128; o++)
			if (((m[o >> 5] >> (o & 31)) & 1u) != (uint32_t)(count[o] <= limit) && failures++ < 20)
				printf("le_coded_filter (%s): limit %u offset %u count %u\n", what, limit, o, count[o]);
	}
}

int main()
{
	check_add<1>();
	check_add<2>();
	check_add<3>();
	check_add<4>();
	check_add<5>();
	check_add<6>();
	check_add<7>();
	check_add<8>();
	check_le();
	uint32_t D[16];
	for (int trial = 0; trial < 200; trial++) {
		for (int d = 0; d < 16; d++)
			D[d] = rnd();
		check_filter(D, "random");
	}
	// a pattern-like stream (groups of 0011 / 1100 at every phase, so counts reach 0) with a few symbols flipped
	for (int trial = 0; trial < 400; trial++) {
		const uint32_t phase = (uint32_t)trial & 3;
		for (int d = 0; d < 16; d++)
			D[d] = 0;
		for (uint32_t x = 0; x < 512; x++) {
			const uint32_t g = (x + phase) >> 2, j = (x + phase) & 3;
			const uint32_t bit = ((g * 2654435761u) >> 13) & 1u;
			D[x >> 5] |= (bit ^ (j >> 1)) << (x & 31);
		}
		for (int f = 0; f < trial / 4; f++)
			D[rnd() & 15] ^= 1u << (rnd() & 31);
		check_filter(D, "groups");
	}
	for (int d = 0; d < 16; d++)
		D[d] = 0;
	check_filter(D, "zeros");                               // every pair equal: 160 everywhere
	for (int d = 0; d < 16; d++)
		D[d] = 0xccccccccu;
	check_filter(D, "0011 repeated");                       // 0 at phase 0 and 2 ... 160 in between
	printf("%d failing cases\n", failures);
	return failures > 255 ? 255 : failures;
}
