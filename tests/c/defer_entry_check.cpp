// Host check of libbtbb_amd/csrc/defer_entry.h: entries packed over the extremes and a seeded sample of every field, every
// accessor against the layout's shifts written out here as literals (the ones the kernels carried before the header existed),
// and the round trip.  Built by tests/test_defer_entry.py with the system g++; prints one line per failing case and their number.
#include <stdio.h>
#include <stdint.h>
#include "../../libbtbb_amd/csrc/defer_entry.h"

static int failures = 0;

static void expect(const char *what, uint64_t got, uint64_t want, uint64_t a, uint64_t b)
{
	if (got != want && failures++ < 20)
		printf("%s: got %llx, want %llx (a %016llx b %016llx)\n", what, (unsigned long long)got, (unsigned long long)want,
		       (unsigned long long)a, (unsigned long long)b);
}

static void check(uint64_t src, uint32_t nw, uint32_t sh, uint32_t pkt, uint32_t len, uint32_t nbits, uint32_t kind, uint32_t wht,
		  uint32_t widx, uint32_t uap)
{
	const uint64_t a = DEFER_PACK_A(src, nw, sh), b = DEFER_PACK_B(pkt, len, nbits, kind, wht, widx, uap);
	// the words, field by field, as literal shifts
	expect("word a", a, src | (uint64_t)nw << 48 | (uint64_t)sh << 55, a, b);
	expect("word b", b, (uint64_t)pkt | (uint64_t)len << 8 | (uint64_t)nbits << 20 | (uint64_t)kind << 32 | (uint64_t)wht << 34 |
				    (uint64_t)widx << 35 | (uint64_t)uap << 42, a, b);
	// the accessors against literal shifts of the words
	expect("src", DEFER_SRC(a), a & 0xffffffffffffULL, a, b);
	expect("nw", DEFER_NW(a), (uint32_t)(a >> 48) & 127u, a, b);
	expect("sh", DEFER_SH(a), (uint32_t)(a >> 55) & 63u, a, b);
	expect("pkt", DEFER_PKT(b), (uint32_t)b & 0xffu, a, b);
	expect("len", DEFER_LEN(b), (uint32_t)(b >> 8) & 0xfffu, a, b);
	expect("nbits", DEFER_NBITS(b), (uint32_t)(b >> 20) & 0xfffu, a, b);
	expect("kind", DEFER_KIND(b), (uint32_t)(b >> 32) & 3u, a, b);
	expect("whitened", DEFER_WHITENED(b), (b >> 34) & 1u, a, b);
	expect("widx", DEFER_WIDX(b), (uint32_t)(b >> 35) & 127u, a, b);
	expect("uap", DEFER_UAP(b), (uint32_t)(b >> 42) & 0xffu, a, b);
	expect("nbits (low dword)", DEFER_NBITS_LO((uint32_t)b), ((uint32_t)b >> 20) & 0xfffu, a, b);
	expect("kind (high dword)", DEFER_KIND_HI((uint32_t)(b >> 32)), (uint32_t)(b >> 32) & 3u, a, b);
	// the round trip
	expect("src back", DEFER_SRC(a), src, a, b);
	expect("nw back", DEFER_NW(a), nw, a, b);
	expect("sh back", DEFER_SH(a), sh, a, b);
	expect("pkt back", DEFER_PKT(b), pkt, a, b);
	expect("len back", DEFER_LEN(b), len, a, b);
	expect("nbits back", DEFER_NBITS(b), nbits, a, b);
	expect("kind back", DEFER_KIND(b), kind, a, b);
	expect("whitened back", DEFER_WHITENED(b), wht, a, b);
	expect("widx back", DEFER_WIDX(b), widx, a, b);
	expect("uap back", DEFER_UAP(b), uap, a, b);
	expect("nbits back (low dword)", DEFER_NBITS_LO((uint32_t)b), nbits, a, b);
	expect("kind back (high dword)", DEFER_KIND_HI((uint32_t)(b >> 32)), kind, a, b);
}

static uint64_t rng = 0x9e3779b97f4a7c15ULL;
static uint64_t next(uint64_t bound)                      // xorshift64*, value in 0 .. bound - 1
{
	rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
	return ((rng * 0x2545f4914f6cdd1dULL) >> 11) % bound;
}

int main()
{
	static const uint32_t kinds[4] = {DHL_DH, DHL_DM, DHL_EV4, DHL_EV5};
	if (DHL_DH != 0u || DHL_DM != 1u || DHL_EV4 != 2u || DHL_EV5 != 3u)
		failures++, printf("the four kinds are not 0 .. 3\n");
	// one field at an extreme, the others at zero and at their maxima
	const uint64_t hi[10] = {(1ULL << 48) - 1, 127, 63, 255, 3125, 4095, 3, 1, 126, 255};
	for (int f = 0; f < 10; f++)
		for (int others = 0; others < 2; others++)
			for (int mine = 0; mine < 2; mine++) {
				uint64_t v[10];
				for (int k = 0; k < 10; k++)
					v[k] = k == f ? (mine ? hi[k] : 0) : (others ? hi[k] : 0);
				check(v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6], (uint32_t)v[7],
				      (uint32_t)v[8], (uint32_t)v[9]);
			}
	// a seeded sample of every field over its whole range
	for (int i = 0; i < 200000; i++)
		check(next(1ULL << 48), (uint32_t)next(128), (uint32_t)next(64), (uint32_t)next(256), (uint32_t)next(3126), (uint32_t)next(4096),
		      kinds[next(4)], (uint32_t)next(2), (uint32_t)next(127), (uint32_t)next(256));
	printf("%d failing cases\n", failures);
	return failures ? 1 : 0;
}
