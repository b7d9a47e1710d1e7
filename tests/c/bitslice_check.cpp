// Host check of the bit-sliced "mismatch count <= limit" networks that ship in libbtbb_amd/csrc/bitslice.h: every network over
// every value of its planes, against the plain count.  A 32-bit plane word carries 32 inputs, so 2^16 inputs are 2048 calls.
// Built by tests/test_bitslice_networks.py with the system g++; prints one line per failing case and returns their number.
#include <stdio.h>
#include "../../libbtbb_amd/csrc/bitslice.h"

static int failures = 0;

// plane k of the 32 inputs base .. base + 31 = bit k of each input
static void planes_of(uint32_t base, int n, uint32_t *P)
{
	for (int k = 0; k < n; k++) {
		P[k] = 0;
		for (uint32_t p = 0; p < 32; p++)
			P[k] |= (((base + p) >> k) & 1u) << p;
	}
}

// offsets of `base` whose input differs from `pattern` in at most `limit` of the n planes
static uint32_t count_le(uint32_t base, int n, uint32_t pattern, int limit)
{
	uint32_t out = 0;
	for (uint32_t p = 0; p < 32; p++)
		out |= (uint32_t)(__builtin_popcount(((base + p) ^ pattern) & ((1u << n) - 1)) <= limit) << p;
	return out;
}

static void report(const char *what, int cls_or_pat, uint32_t pattern, int limit, uint32_t base, uint32_t got, uint32_t want)
{
	if (got != want && failures++ < 20)
		printf("%s<%d> pattern %04x limit %d inputs %u..: %08x, count says %08x\n", what, cls_or_pat, pattern, limit, base, got, want);
}

// known LAP: plane k of top16_filter = sync-word bit 24 + k (k < 8) / 48 + k; planes 9 .. 15 are the class bits 57 .. 63, which a
// class-specialised instance takes from barker_bit instead of flip[]
template <int CLS>
static void check_known(uint32_t free_bits)
{
	uint32_t pat16 = free_bits & 0x1ff, flip[16], P[16];
	for (int j = 0; j < 7; j++)
		pat16 |= (CLS < 0 ? (free_bits >> (9 + j)) & 1u : (uint32_t)barker_bit(CLS, j)) << (9 + j);
	for (int k = 0; k < 16; k++)
		flip[k] = ((pat16 >> k) & 1) ? 0xffffffffu : 0u;
	const int limits[] = { 0, 1, 2, 3, 4, 5, 16 };
	for (int limit : limits) {
		for (uint32_t base = 0; base < (1u << 16); base += 32) {
			planes_of(base, 16, P);
			report("top16_filter", CLS, pat16, limit, base, top16_filter<CLS>(P, P + 8, flip, limit), count_le(base, 16, pat16, limit));
		}
		// top12_filter: planes 0 .. 3 = lowp[4 .. 7], 4 .. 11 = highp[0 .. 7], their pattern bits flip[4 ..]
		const uint32_t pat12 = pat16 >> 4;
		const int limit12 = limit == 16 ? 12 : limit;
		for (uint32_t base = 0; base < (1u << 12); base += 32) {
			uint32_t Q[16] = { 0 };
			planes_of(base, 12, Q + 4);
			report("top12_filter", CLS, pat12, limit12, base, top12_filter<CLS>(Q, Q + 8, flip, limit12), count_le(base, 12, pat12, limit12));
		}
	}
}

template <int PAT, int LIMIT>
static void check_le_one(uint32_t pattern)
{
	uint32_t flip[16], P[16];
	for (int k = 0; k < 16; k++)
		flip[k] = ((pattern >> k) & 1) ? 0xffffffffu : 0u;
	for (uint32_t base = 0; base < (1u << 16); base += 32) {
		planes_of(base, 16, P);
		report("le_filter16", PAT, pattern, LIMIT, base, le_filter16<PAT, LIMIT>(P, flip), count_le(base, 16, pattern, LIMIT));
	}
}
template <int PAT>
static void check_le(uint32_t pattern)
{
	check_le_one<PAT, 0>(pattern);
	check_le_one<PAT, 1>(pattern);
	check_le_one<PAT, 2>(pattern);
	check_le_one<PAT, 3>(pattern);
	check_le_one<PAT, 4>(pattern);
}

int main()
{
	constexpr int ADV_PAT = 0xaa | (0x8e << 8);         // the advertising AA's sixteen filter bits, as le.hip folds them
	uint32_t r = 0x2545f491u;
	for (int trial = 0; trial < 6; trial++) {           // patterns: all zeros, all ones, four xorshift words
		const uint32_t pattern = trial == 0 ? 0u : trial == 1 ? 0xffffu : (r & 0xffffu);
		r ^= r << 13, r ^= r >> 17, r ^= r << 5;
		check_known<-1>(pattern);
		check_known<0>(pattern);
		check_known<1>(pattern);
		check_le<-1>(pattern);
	}
	check_le<ADV_PAT>(ADV_PAT);
	printf("%d failing cases\n", failures);
	return failures ? 1 : 0;
}
