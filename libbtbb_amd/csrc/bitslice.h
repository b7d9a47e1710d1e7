// bitslice.h -- bit-slice primitives and the three "mismatch count <= limit" networks of the pattern scans (scan_known.h: known
// LAP, le.hip: LE access address).  A 32-bit word is one plane: bit p belongs to offset p of a chain of 32 offsets.
// For the device the primitives are the gfx950 instructions the kernels were measured with; for the host (no HIP headers
// needed) plain C++ with the same results: tests/c/bitslice_check.cpp runs the networks that ship over every input.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BITSLICE_FN __device__ __forceinline__
#else
#define BITSLICE_FN static inline
#endif

#define BARKER1   0x27u                    // 7-bit window when LAP bit 23 = 1 (host order)
#define BARKER0   0x58u                    // 7-bit window when LAP bit 23 = 0

// alignbit: bits sh .. sh + 31 of hi:lo (v_alignbit: the low five bits of sh count)
// lowest_bit: index of the lowest set bit; 0xffffffff for 0 (v_ffbl_b32), which the callers use as "offset 31 of a lane that
// has nothing left" -- its result is masked out afterwards
// bitop3: three-input boolean in one full-rate instruction (truth table index = a*4 + b*2 + c); the table of v_bitop3 is an
// immediate, so it has to reach the builtin as a template constant
#ifdef __HIPCC__
BITSLICE_FN uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
BITSLICE_FN uint32_t lowest_bit(uint32_t m)
{
	uint32_t p;
	asm("v_ffbl_b32 %0, %1" : "=v"(p) : "v"(m));
	return p;
}
template <uint32_t TT>
BITSLICE_FN uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, TT); }
#else
BITSLICE_FN uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31)); }
BITSLICE_FN uint32_t lowest_bit(uint32_t m) { return m ? (uint32_t)__builtin_ctz(m) : 0xffffffffu; }
template <uint32_t TT>
BITSLICE_FN uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c)
{
	uint32_t r = 0;
	for (uint32_t idx = 0; idx < 8; idx++)
		if ((TT >> idx) & 1)
			r |= ((idx & 4) ? a : ~a) & ((idx & 2) ? b : ~b) & ((idx & 1) ? c : ~c);
	return r;
}
#endif
#define BITOP3(a, b, c, tt) bitop3<(tt)>((a), (b), (c))
BITSLICE_FN uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return bitop3<0x96>(a, b, c); }
#define FA_SUM(a, b, c) BITOP3((a), (b), (c), 0x96)        // full adder: sum ...
#define FA_CARRY(a, b, c) BITOP3((a), (b), (c), 0xe8)      // ... and carry (majority)

// Truth table of f(a ^ ia, b ^ ib, c ^ ic) for the table `base` of f(a, b, c): a pattern bit that is known at compile time
// goes into the adder's immediate instead of costing an XOR per plane.
// Known LAP: the sync word's top seven bits are the LAP's MSB and the barker code that follows from it
// (bluetooth_packet.c:81-113), so for a given class the mismatch planes of window bits 57..63 are the stream planes themselves
// or their complements (CLS = 0 / 1; -1 = every plane XORed with its run-time flip mask).  LE: the sixteen filter bits of the
// advertising access address.
constexpr uint32_t tt3(uint32_t base, bool ia, bool ib, bool ic)
{
	uint32_t t = 0;
	for (uint32_t idx = 0; idx < 8; idx++) {
		const uint32_t a = ((idx >> 2) & 1) ^ (ia ? 1u : 0u), b = ((idx >> 1) & 1) ^ (ib ? 1u : 0u), c = (idx & 1) ^ (ic ? 1u : 0u);
		t |= ((base >> (a * 4 + b * 2 + c)) & 1) << idx;
	}
	return t;
}
// sync-word bit 57 + j of class CLS: 0x27 = 0100111b for LAP MSB 1, its complement for 0
constexpr bool barker_bit(int cls, int j) { return (((cls ? BARKER1 : BARKER0) >> j) & 1) != 0; }

// The planes of the known-LAP filters (round 6, late): the filter may count mismatches in ANY subset of the sync word's bits, so it
// takes them where the funnel shifts can be shared -- window bits 24 + j and 56 + j (j = 0 .. 7) of the offsets p of a 32-offset half
// are the stream bits p + 24 + j of two neighbouring dword pairs, and the UPPER planes of one half are the LOWER planes of the next:
// three sets of eight shifts per word instead of four (sixteen top bits per half: 32 v_alignbit per word -> 24).  Bits 57 .. 63 are
// still the class bits whose complement folds into the adders' truth tables.
// P[j] = stream bit p + 24 + j of hi:lo for the 32 offsets p of a half (j = FIRST .. 7)
template <int FIRST>
BITSLICE_FN void pair_planes(uint32_t lo, uint32_t hi, uint32_t *P)
{
#pragma unroll
	for (int j = FIRST; j < 8; j++)
		P[j] = alignbit(hi, lo, 24 + j);
}

// bit-sliced "mismatches in sync-word bits 28..31 and 56..63 <= limit" for 32 offsets: twelve planes
// (lowp[4 .. 7] = window bits 28 .. 31, highp[0 .. 7] = window bits 56 .. 63; flip[4 + k] = the sync word's bit of plane k),
// a carry-save adder tree to a 4-bit count per offset, and a bit-sliced compare with the run-time limit.  For limit 2 it keeps
// 79 / 4096 = 1.9 % of the offsets of a random stream.
template <int CLS>
BITSLICE_FN uint32_t top12_filter(const uint32_t *lowp, const uint32_t *highp, const uint32_t *flip, int limit)
{
	if (limit >= 12)
		return 0xffffffffu;
	uint32_t m[12];
#pragma unroll
	for (int k = 0; k < 12; k++) {                      // plane k: 0 .. 3 = window bits 28 .. 31, 4 = bit 56, 5 .. 11 = the class bits 57 .. 63
		m[k] = k < 4 ? lowp[4 + k] : highp[k - 4];
		if (CLS < 0 || k < 5)
			m[k] ^= flip[4 + k];
	}
	constexpr bool K = CLS >= 0;
#define INV(k) (K && barker_bit(CLS, (k) - 5))
	if (limit == 0) {                                   // no mismatch at all: the OR of the twelve planes (six instructions; third session of round 6)
		const uint32_t r0 = BITOP3(m[0], m[1], m[2], 0xfe);
		const uint32_t r1 = bitop3<tt3(0xfe, false, false, INV(5))>(m[3], m[4], m[5]);
		const uint32_t r2 = bitop3<tt3(0xfe, INV(6), INV(7), INV(8))>(m[6], m[7], m[8]);
		const uint32_t r3 = bitop3<tt3(0xfe, INV(9), INV(10), INV(11))>(m[9], m[10], m[11]);
		return ~(BITOP3(r0, r1, r2, 0xfe) | r3);
	}
	const uint32_t s0 = FA_SUM(m[0], m[1], m[2]), c0 = FA_CARRY(m[0], m[1], m[2]);
	const uint32_t s1 = bitop3<tt3(0x96, false, false, INV(5))>(m[3], m[4], m[5]), c1 = bitop3<tt3(0xe8, false, false, INV(5))>(m[3], m[4], m[5]);
	const uint32_t s2 = bitop3<tt3(0x96, INV(6), INV(7), INV(8))>(m[6], m[7], m[8]), c2 = bitop3<tt3(0xe8, INV(6), INV(7), INV(8))>(m[6], m[7], m[8]);
	const uint32_t s3 = bitop3<tt3(0x96, INV(9), INV(10), INV(11))>(m[9], m[10], m[11]), c3 = bitop3<tt3(0xe8, INV(9), INV(10), INV(11))>(m[9], m[10], m[11]);
#undef INV
	const uint32_t o1 = FA_SUM(s0, s1, s2), k0 = FA_CARRY(s0, s1, s2);
	if (limit == 1) {                                   // count = o1 + s3 + 2 x (c0 .. c3, k0): <= 1 <=> none of those five and not both of o1, s3
		const uint32_t w = BITOP3(c0, c1, c2, 0xfe);
		const uint32_t x = BITOP3(c3, k0, w, 0xfe);
		return ~BITOP3(x, o1, s3, 0xf8);                // ~(x | (o1 & s3))
	}
	const uint32_t ones = o1 ^ s3, k1 = o1 & s3;
	const uint32_t t0 = FA_SUM(c0, c1, c2), f0 = FA_CARRY(c0, c1, c2);
	const uint32_t t1 = FA_SUM(c3, k0, k1), f1 = FA_CARRY(c3, k0, k1);
	const uint32_t twos = t0 ^ t1, f2 = t0 & t1;
	if (limit <= 3) {                                   // (see top16_filter)
		const uint32_t ge4 = BITOP3(f0, f1, f2, 0xfe);
		const uint32_t low = limit == 0 ? (twos | ones) : limit == 1 ? twos : limit == 2 ? (twos & ones) : 0u;
		return ~(ge4 | low);
	}
	const uint32_t fours = FA_SUM(f0, f1, f2), eights = FA_CARRY(f0, f1, f2);
	// count = ones + 2 twos + 4 fours + 8 eights; keep offsets with count <= limit
	uint32_t gt = 0, eq = 0xffffffffu;
	const uint32_t planes[4] = { eights, fours, twos, ones };
#pragma unroll
	for (int b = 0; b < 4; b++) {
		const uint32_t lim_bit = ((limit >> (3 - b)) & 1) ? 0xffffffffu : 0u;
		gt |= eq & planes[b] & ~lim_bit;
		eq &= ~(planes[b] ^ lim_bit);
	}
	return ~gt;
}

// The same over sixteen sync-word bits (24..31 and 56..63): five more adders, but for limit >= 2 it
// leaves a tenth of the survivors (0.2 % instead of 1.9 % at limit 2), which is worth more than it
// costs; for limit <= 1 the twelve-plane filter is already sparse enough and cheaper.
template <int CLS>
BITSLICE_FN uint32_t top16_filter(const uint32_t *lowp, const uint32_t *highp, const uint32_t *flip, int limit)
{
	if (limit >= 16)
		return 0xffffffffu;
	uint32_t m[16];
#pragma unroll
	for (int k = 0; k < 16; k++) {                      // plane k: 0 .. 7 = window bits 24 .. 31, 8 = bit 56, 9 .. 15 = the class bits 57 .. 63
		m[k] = k < 8 ? lowp[k] : highp[k - 8];
		if (CLS < 0 || k < 9)
			m[k] ^= flip[k];
	}
	constexpr bool K = CLS >= 0;
#define INV(k) (K && barker_bit(CLS, (k) - 9))
	// weight 1
	const uint32_t s0 = FA_SUM(m[0], m[1], m[2]), c0 = FA_CARRY(m[0], m[1], m[2]);
	const uint32_t s1 = FA_SUM(m[3], m[4], m[5]), c1 = FA_CARRY(m[3], m[4], m[5]);
	const uint32_t s2 = FA_SUM(m[6], m[7], m[8]), c2 = FA_CARRY(m[6], m[7], m[8]);
	const uint32_t s3 = bitop3<tt3(0x96, INV(9), INV(10), INV(11))>(m[9], m[10], m[11]), c3 = bitop3<tt3(0xe8, INV(9), INV(10), INV(11))>(m[9], m[10], m[11]);
	const uint32_t s4 = bitop3<tt3(0x96, INV(12), INV(13), INV(14))>(m[12], m[13], m[14]), c4 = bitop3<tt3(0xe8, INV(12), INV(13), INV(14))>(m[12], m[13], m[14]);
	const uint32_t o1 = FA_SUM(s0, s1, s2), k0 = FA_CARRY(s0, s1, s2);
	const uint32_t o2 = bitop3<tt3(0x96, false, false, INV(15))>(s3, s4, m[15]), k1 = bitop3<tt3(0xe8, false, false, INV(15))>(s3, s4, m[15]);
#undef INV
	// limit 2 or 3 (third session of round 6): count = o1 + o2 + 2 x (bits set among W = c0 .. c4, k0, k1), so
	//   count <= 2  <=>  no bit of W, or exactly one and neither o1 nor o2     = at_most_one(W) & ~(any(W) & (o1 | o2))
	//   count <= 3  <=>  no bit of W, or exactly one and not both o1 and o2    = at_most_one(W) & ~(any(W) & o1 & o2)
	// at_most_one over the groups (c0 c1 c2) (c3 c4 k0) (k1): no group holds two, no two groups hold one -- nine instructions
	// where the twos / fours columns, their carries and the compare took thirteen (27 -> 23 per 32 offsets)
	if (limit == 2 || limit == 3) {
		const uint32_t a0 = BITOP3(c0, c1, c2, 0xfe), t0 = BITOP3(c0, c1, c2, 0xe8);     // any / at least two of a group
		const uint32_t a1 = BITOP3(c3, c4, k0, 0xfe), t1 = BITOP3(c3, c4, k0, 0xe8);
		const uint32_t two_groups = BITOP3(a0, a1, k1, 0xe8);
		const uint32_t any = BITOP3(a0, a1, k1, 0xfe);
		const uint32_t odd = limit == 2 ? BITOP3(any, o1, o2, 0xe0)                       // any & (o1 | o2)
						: BITOP3(any, o1, o2, 0x80);                      // any & o1 & o2
		const uint32_t bad = BITOP3(t0, t1, two_groups, 0xfe);
		return ~(bad | odd);
	}
	const uint32_t ones = o1 ^ o2, k2 = o1 & o2;
	// weight 2: c0..c4, k0, k1, k2
	const uint32_t t0 = FA_SUM(c0, c1, c2), f0 = FA_CARRY(c0, c1, c2);
	const uint32_t t1 = FA_SUM(c3, c4, k0), f1 = FA_CARRY(c3, c4, k0);
	const uint32_t t2 = FA_SUM(k1, k2, t0), f2 = FA_CARRY(k1, k2, t0);
	const uint32_t twos = t1 ^ t2, f3 = t1 & t2;
	// limit <= 3: "count >= 4" is all that matters of the upper weights, and it is the OR of the four carries out of the
	// twos column -- six adder instructions and the compare become three (the compiler cannot find this: it is not the
	// same function as the sum it replaces)
	if (limit <= 3) {
		const uint32_t ge4 = BITOP3(f0, f1, f2, 0xfe);
		const uint32_t low = limit == 0 ? (twos | ones) : limit == 1 ? twos : limit == 2 ? (twos & ones) : 0u;
		return ~BITOP3(ge4, f3, low, 0xfe);
	}
	// weight 4: f0..f3
	const uint32_t g0 = FA_SUM(f0, f1, f2), h0 = FA_CARRY(f0, f1, f2);
	const uint32_t fours = g0 ^ f3, h1 = g0 & f3;
	// weight 8, 16
	const uint32_t eights = h0 ^ h1, sixteens = h0 & h1;
	// count = ones + 2 twos + 4 fours + 8 eights + 16 sixteens; keep offsets with count <= limit
	uint32_t gt = sixteens, eq = ~sixteens;
	const uint32_t planes[4] = { eights, fours, twos, ones };
#pragma unroll
	for (int b = 0; b < 4; b++) {
		const uint32_t lim_bit = ((limit >> (3 - b)) & 1) ? 0xffffffffu : 0u;
		gt |= eq & planes[b] & ~lim_bit;
		eq &= ~(planes[b] ^ lim_bit);
	}
	return ~gt;
}

// Bit-sliced pre-filter over sixteen of the forty pattern bits: window bits 0..7 (the preamble) and 32..39 (the AA's
// last octet) of 32 offsets.  r[0..7] = window bits 0..7, r[8..15] = bits 32..39.  PAT >= 0: the sixteen pattern bits
// (bit k = plane k) are folded into the first adder level; PAT < 0: flip[k] (all ones where the pattern has a 1) is
// XORed into each plane.  Returns the offsets with at most `limit` mismatches among the sixteen -- the count itself is
// never formed: weight-1 sums s*, weight-2 carries c*; count = ones + 2 T with T = the number of set weight-2 bits, and
// "<= limit" is decided from whether T is 0, <= 1 or <= 2.
template <int PAT, int LIMIT>
BITSLICE_FN uint32_t le_filter16(const uint32_t *r, const uint32_t *flip)
{
	uint32_t m[16];
#pragma unroll
	for (int k = 0; k < 16; k++)
		m[k] = PAT < 0 ? (r[k] ^ flip[k]) : r[k];
#define INV(k) (PAT >= 0 && ((PAT >> (k)) & 1))
#define G3(base, i) bitop3<tt3(base, INV(i), INV(i + 1), INV(i + 2))>(m[i], m[i + 1], m[i + 2])
	const uint32_t m15 = INV(15) ? ~m[15] : m[15];
	if (LIMIT == 0) {                                   // no mismatch: the NOR of the sixteen planes
		const uint32_t x0 = G3(0xfe, 0), x1 = G3(0xfe, 3), x2 = G3(0xfe, 6), x3 = G3(0xfe, 9), x4 = G3(0xfe, 12);
		return ~(bitop3<0xfe>(x0, x1, x2) | bitop3<0xfe>(x3, x4, m15));
	}
	const uint32_t s0 = G3(0x96, 0), c0 = G3(0xe8, 0);
	const uint32_t s1 = G3(0x96, 3), c1 = G3(0xe8, 3);
	const uint32_t s2 = G3(0x96, 6), c2 = G3(0xe8, 6);
	const uint32_t s3 = G3(0x96, 9), c3 = G3(0xe8, 9);
	const uint32_t s4 = G3(0x96, 12), c4 = G3(0xe8, 12);
#undef G3
#undef INV
	const uint32_t o1 = bitop3<0x96>(s0, s1, s2), k0 = bitop3<0xe8>(s0, s1, s2);
	const uint32_t o2 = bitop3<0x96>(s3, s4, m15), k1 = bitop3<0xe8>(s3, s4, m15);
	const uint32_t ones = o1 ^ o2, k2 = o1 & o2;
	// the eight weight-2 bits c0..c4, k0, k1, k2 in three groups: a* = sums, b* = carries (weight 4 in the count)
	if (LIMIT == 1)                                     // T == 0
		return ~(bitop3<0xfe>(bitop3<0xfe>(c0, c1, c2), bitop3<0xfe>(c3, c4, k0), k1) | k2);
	const uint32_t a0 = bitop3<0x96>(c0, c1, c2), b0 = bitop3<0xe8>(c0, c1, c2);
	const uint32_t a1 = bitop3<0x96>(c3, c4, k0), b1 = bitop3<0xe8>(c3, c4, k0);
	const uint32_t a2 = k1 ^ k2, b2 = k1 & k2;
	const uint32_t b_any = bitop3<0xfe>(b0, b1, b2);
	const uint32_t le1 = ~(b_any | bitop3<0xe8>(a0, a1, a2));                          // T <= 1
	if (LIMIT == 3)
		return le1;
	if (LIMIT == 2) {                                   // T == 0, or T == 1 and no weight-1 mismatch
		const uint32_t z = ~(b_any | bitop3<0xfe>(a0, a1, a2));
		return z | (le1 & ~ones);
	}
	// LIMIT 4: T <= 1, or T == 2 and no weight-1 mismatch.  T <= 2 <=> (no b and not all three a) or (exactly one b and no a)
	const uint32_t b_one = bitop3<0x96>(b0, b1, b2) & ~bitop3<0xe8>(b0, b1, b2);
	const uint32_t le2 = (~b_any & ~bitop3<0x80>(a0, a1, a2)) | (b_one & ~bitop3<0xfe>(a0, a1, a2));
	return le1 | (le2 & ~ones);
}

// ---- LE Coded PHY (le_coded.h): bit-sliced counters wider than a handful of planes ----
// bs_add<N>: o[0 .. N] = a[0 .. N-1] + b[0 .. N-1], planes LSB first (a ripple of full adders: two instructions per plane).
// o must not alias a or b.
template <int N>
BITSLICE_FN void bs_add(const uint32_t *a, const uint32_t *b, uint32_t *o)
{
	uint32_t c = a[0] & b[0];
	o[0] = a[0] ^ b[0];
#pragma unroll
	for (int k = 1; k < N; k++) {
		o[k] = FA_SUM(a[k], b[k], c);
		c = FA_CARRY(a[k], b[k], c);
	}
	o[N] = c;
}

// bs_shift_add<N>: o = lo + (the N-plane stream hi:lo moved down by sh positions, 0 < sh < 32): the count at offset p plus the
// count at offset p + sh
template <int N>
BITSLICE_FN void bs_shift_add(const uint32_t *lo, const uint32_t *hi, uint32_t sh, uint32_t *o)
{
	uint32_t s[N];
#pragma unroll
	for (int k = 0; k < N; k++)
		s[k] = alignbit(hi[k], lo[k], sh);
	bs_add<N>(lo, s, o);
}

// bs_le<N>: the offsets whose N-plane count is <= limit (a run-time value below 2^N)
template <int N>
BITSLICE_FN uint32_t bs_le(const uint32_t *p, uint32_t limit)
{
	uint32_t gt = 0, eq = 0xffffffffu;
#pragma unroll
	for (int b = N - 1; b >= 0; b--) {
		const uint32_t lim_bit = ((limit >> b) & 1) ? 0xffffffffu : 0u;
		gt |= eq & p[b] & ~lim_bit;
		eq &= ~(p[b] ^ lim_bit);
	}
	return ~gt;
}

// The coded scan's necessary condition.  Preamble and mapped access address are 84 groups of four symbols, each 0011 or 1100,
// whatever the address: symbols k and k + 2 of the pattern differ for k mod 4 in {0, 1}.  These 168 pairs are disjoint, so a
// window with e mismatches has at most e pairs of EQUAL symbols, and "equal pairs among the first 160 (groups 0 .. 79, window
// symbols 0 .. 319) <= limit" can never reject a match.  Per dword d of the stream: V = pairs that are equal, A = V + V >> 1 (a
// group's two pairs), then + >> 4, + >> 8, + >> 16: B[d] = the equal pairs of the eight groups from each of its 32 offsets;
// chain c (the 32 offsets from dword c) sums B[c .. c + 9] as (c, c+1) + (c+2, c+3) + ... pairwise, every partial sum shared with the
// neighbouring chains.  D[0 .. 15]: the sixteen dwords from the first chain's; m[0 .. 3]: the surviving offsets of four chains.
// About 900 instructions for 128 offsets.  On a random stream the count is binomial(160, 1/2).
#define LE_CODED_FILTER_PAIRS 160
BITSLICE_FN void le_coded_filter(const uint32_t *D, uint32_t limit, uint32_t *m)
{
	uint32_t V[15], A[15][2], A4[15][3], A8[15][4], B[13][5], C[12][6], E[8][7], G[4][8];
#pragma unroll
	for (int d = 0; d < 15; d++)
		V[d] = ~(D[d] ^ alignbit(D[d + 1], D[d], 2));
#pragma unroll
	for (int d = 0; d < 14; d++)
		bs_shift_add<1>(&V[d], &V[d + 1], 1, A[d]);
	A[14][0] = A[14][1] = 0;                            // (dword 14 of A, A4 and A8 only feeds bits of dword 13 that nothing reads)
#pragma unroll
	for (int d = 0; d < 14; d++)
		bs_shift_add<2>(A[d], A[d + 1], 4, A4[d]);
	A4[14][0] = A4[14][1] = A4[14][2] = 0;
#pragma unroll
	for (int d = 0; d < 14; d++)
		bs_shift_add<3>(A4[d], A4[d + 1], 8, A8[d]);
#pragma unroll
	for (int d = 0; d < 13; d++)
		bs_shift_add<4>(A8[d], A8[d + 1], 16, B[d]);
#pragma unroll
	for (int d = 0; d < 12; d++)
		bs_add<5>(B[d], B[d + 1], C[d]);
#pragma unroll
	for (int d = 0; d < 8; d++)
		bs_add<6>(C[d], C[d + 2], E[d]);
#pragma unroll
	for (int c = 0; c < 4; c++) {
		bs_add<7>(E[c], E[c + 4], G[c]);
		uint32_t last[8], sum[9];
#pragma unroll
		for (int k = 0; k < 8; k++)
			last[k] = k < 6 ? C[c + 8][k] : 0u;
		bs_add<8>(G[c], last, sum);                     // (at most 160: sum[8] is never set)
		m[c] = bs_le<8>(sum, limit);
	}
}
