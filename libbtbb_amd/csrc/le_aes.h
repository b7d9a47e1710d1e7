// le_aes.h -- AES-128 encryption for the LE stages (included by le_crypt.h and le_pair.h): one round table in LDS,
// te[x] = 2s | s << 8 | s << 16 | 3s << 24 with s = S(x); a block is four little-endian words.  Nothing here knows a stage's arguments:
// the table is built by lx_te_entry, one entry per thread, and every function takes it as a pointer.
#pragma once

#define LX_RK        44u                   // words of an AES-128 key schedule

__device__ __forceinline__ uint32_t lx_rotl(uint32_t v, uint32_t s) { return (v << s) | (v >> (32u - s)); }

__device__ __forceinline__ uint32_t lx_gmul(uint32_t x, uint32_t y)
{
	uint32_t r = 0;
	for (int j = 0; j < 8; j++) {
		if (y & 1u)
			r ^= x;
		x = (x << 1) ^ ((x & 0x80u) ? 0x11bu : 0u);
		y >>= 1;
	}
	return r;
}

// the S-box from its definition: the inverse in GF(2^8) modulo x^8 + x^4 + x^3 + x + 1, then the affine map
__device__ __forceinline__ uint32_t lx_te_entry(uint32_t x)
{
	uint32_t inv = 0;
	for (uint32_t y = 1; y < 256; y++)
		if (lx_gmul(x, y) == 1u)
			inv = y;
	const uint32_t w = inv | (inv << 8);
	const uint32_t s = (inv ^ (w >> 7) ^ (w >> 6) ^ (w >> 5) ^ (w >> 4) ^ 0x63u) & 0xffu;
	const uint32_t s2 = lx_gmul(s, 2);
	return s2 | (s << 8) | (s << 16) | ((s2 ^ s) << 24);
}

__device__ __forceinline__ uint32_t lx_sub(const uint32_t *te, uint32_t x) { return (te[x] >> 8) & 0xffu; }

__device__ __forceinline__ uint32_t lx_sub_word(const uint32_t *te, uint32_t w)
{
	return lx_sub(te, w & 0xffu) | (lx_sub(te, (w >> 8) & 0xffu) << 8) | (lx_sub(te, (w >> 16) & 0xffu) << 16) | (lx_sub(te, w >> 24) << 24);
}

// rk[0..3] = the key -> the schedule
__device__ __forceinline__ void lx_expand(const uint32_t *te, uint32_t (&rk)[LX_RK])
{
	uint32_t rc = 1;
#pragma unroll
	for (int i = 4; i < (int)LX_RK; i++) {
		uint32_t t = rk[i - 1];
		if ((i & 3) == 0) {
			t = lx_sub_word(te, (t >> 8) | (t << 24)) ^ rc;
			rc = ((rc << 1) ^ ((rc & 0x80u) ? 0x11bu : 0u)) & 0xffu;
		}
		rk[i] = rk[i - 4] ^ t;
	}
}

struct LxBlock { uint32_t w[4]; };

__device__ __forceinline__ uint32_t lx_col(const uint32_t *te, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
	return te[a & 0xffu] ^ lx_rotl(te[(b >> 8) & 0xffu], 8) ^ lx_rotl(te[(c >> 16) & 0xffu], 16) ^ lx_rotl(te[d >> 24], 24);
}

__device__ __forceinline__ LxBlock lx_aes(const uint32_t *te, const uint32_t (&rk)[LX_RK], const LxBlock &in)
{
	uint32_t s0 = in.w[0] ^ rk[0], s1 = in.w[1] ^ rk[1], s2 = in.w[2] ^ rk[2], s3 = in.w[3] ^ rk[3];
#pragma unroll
	for (int r = 1; r < 10; r++) {
		const uint32_t t0 = lx_col(te, s0, s1, s2, s3) ^ rk[4 * r], t1 = lx_col(te, s1, s2, s3, s0) ^ rk[4 * r + 1];
		const uint32_t t2 = lx_col(te, s2, s3, s0, s1) ^ rk[4 * r + 2], t3 = lx_col(te, s3, s0, s1, s2) ^ rk[4 * r + 3];
		s0 = t0;
		s1 = t1;
		s2 = t2;
		s3 = t3;
	}
	LxBlock o;
	o.w[0] = (lx_sub(te, s0 & 0xffu) | (lx_sub(te, (s1 >> 8) & 0xffu) << 8) | (lx_sub(te, (s2 >> 16) & 0xffu) << 16) | (lx_sub(te, s3 >> 24) << 24)) ^ rk[40];
	o.w[1] = (lx_sub(te, s1 & 0xffu) | (lx_sub(te, (s2 >> 8) & 0xffu) << 8) | (lx_sub(te, (s3 >> 16) & 0xffu) << 16) | (lx_sub(te, s0 >> 24) << 24)) ^ rk[41];
	o.w[2] = (lx_sub(te, s2 & 0xffu) | (lx_sub(te, (s3 >> 8) & 0xffu) << 8) | (lx_sub(te, (s0 >> 16) & 0xffu) << 16) | (lx_sub(te, s1 >> 24) << 24)) ^ rk[42];
	o.w[3] = (lx_sub(te, s3 & 0xffu) | (lx_sub(te, (s0 >> 8) & 0xffu) << 8) | (lx_sub(te, (s1 >> 16) & 0xffu) << 16) | (lx_sub(te, s2 >> 24) << 24)) ^ rk[43];
	return o;
}

__device__ __forceinline__ void lx_load_rk(const uint32_t *sched, uint32_t (&rk)[LX_RK])
{
#pragma unroll
	for (int j = 0; j < (int)LX_RK / 4; j++) {
		const uint4 v = reinterpret_cast<const uint4 *>(sched)[j];
		rk[4 * j] = v.x;
		rk[4 * j + 1] = v.y;
		rk[4 * j + 2] = v.z;
		rk[4 * j + 3] = v.w;
	}
}

__device__ __forceinline__ uint32_t lx_bswap(uint32_t v) { return __builtin_bswap32(v); }
