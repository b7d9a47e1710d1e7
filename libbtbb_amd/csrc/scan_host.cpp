// scan_host.cpp -- the host level of the access-code scan: capture in host memory in, hits in (stream, offset) order out.
// Pure host code: every function here goes through the exported device entries (btbbx_scan_device, btbbx_scan_ordered_device,
// btbbx_pack_device ...: scan.hip, sort.hip) and the call leases of context.cpp; none launches a kernel itself.  Also the
// argument check every scan entry shares (check_scan_args, declared in common.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <thread>
#include <vector>
#include "common.h"

// the checks every scan entry makes of its streams; `window` = bits of the pattern (64: access code, 40: LE preamble + AA)
int check_scan_args(const char *who, int window, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits)
{
	if (n_streams == 0 || n_streams > 65535) {
		set_error("%s: n_streams must be 1..65535", who);
		return BTBBX_E_ARG;
	}
	if (n_streams > 1 && pitch_words < n_words) {
		set_error("%s: pitch_words < n_words", who);
		return BTBBX_E_ARG;
	}
	if (n_words > (1ull << 40) || search_bits + (window - 1) > n_words * 64) {
		set_error("%s: search_bits + %d exceeds the stream (%llu > %llu bits)", who, window - 1,
			  (unsigned long long)(search_bits + (window - 1)), (unsigned long long)(n_words * 64));
		return BTBBX_E_ARG;
	}
	return BTBBX_OK;
}

// (stream, offset) order.  Large lists (a 1 GiB capture yields ~10^6 hits) go through an LSD radix
// sort with 16-bit digits on the key stream << 48 | offset, skipping digits that are equal in all
// keys -- three passes for a 4 GiB stream instead of std::sort's ~20 n comparisons, which used to
// be most of the PCIe-inclusive time of the streaming ingest.
extern "C" void btbbx_sort_hits(btbbx_hit *hits, size_t n)
{
	auto key = [](const btbbx_hit &h) { return ((uint64_t)h.stream << 48) | (h.offset & 0xffffffffffffULL); };
	bool small_offsets = true;
	uint64_t all_or = 0, all_and = ~0ULL;
	for (size_t i = 0; i < n; i++) {
		small_offsets &= (hits[i].offset >> 48) == 0;
		const uint64_t k = key(hits[i]);
		all_or |= k;
		all_and &= k;
	}
	if (n < 4096 || !small_offsets) {
		std::sort(hits, hits + n, [](const btbbx_hit &x, const btbbx_hit &y) {
			if (x.stream != y.stream) return x.stream < y.stream;
			return x.offset < y.offset;
		});
		return;
	}
	std::vector<btbbx_hit> tmp(n);
	std::vector<size_t> count(65536);
	btbbx_hit *src = hits, *dst = tmp.data();
	for (int shift = 0; shift < 64; shift += 16) {
		if ((((all_or ^ all_and) >> shift) & 0xffff) == 0)
			continue;                       // this digit is the same in every key
		std::fill(count.begin(), count.end(), 0);
		for (size_t i = 0; i < n; i++)
			count[(key(src[i]) >> shift) & 0xffff]++;
		size_t run = 0;
		for (size_t d = 0; d < 65536; d++) {
			const size_t c = count[d];
			count[d] = run;
			run += c;
		}
		for (size_t i = 0; i < n; i++)
			dst[count[(key(src[i]) >> shift) & 0xffff]++] = src[i];
		std::swap(src, dst);
	}
	if (src != hits)
		memcpy(hits, src, n * sizeof(btbbx_hit));
}

// Scan words already on the current device and bring the hits back in (stream, offset) order.
// `cap` limits what is WRITTEN, never what is found: when more offsets match than the device buffer
// of the first pass holds, the scan is repeated with a buffer of the size the counter reported, so
// that the records handed back are always the `cap` SMALLEST (stream, offset) ones -- a caller asking
// for one hit gets the first match, as btbb_find_ac would return it (bluetooth_packet.c:444-464).
static int64_t scan_resident(const uint64_t *d_words, uint64_t n_words, uint64_t search_bits, uint32_t lap,
			     int max_ac_errors, btbbx_hit *hits, uint64_t cap, uint64_t offset_base, hipStream_t q)
{
	// counter + records live in one grow-only block of the call's lease (context.cpp scope_hits): no allocation
	// in steady state.  Layout: 16 bytes for the counter, then the records (16-byte aligned).
	struct Dev {
		btbbx_hit *hits = nullptr;
		uint32_t *count = nullptr;
	} d;
	// first guess: room for what the caller can take, but no more than one hit per 256 offsets + slack
	uint64_t guess = search_bits / 256 + 4096;
	if (guess > cap)
		guess = cap;
	uint32_t dev_cap = guess > 0xffffffffULL ? 0xffffffffu : (uint32_t)guess;
	uint32_t count = 0;
	for (int pass = 0; pass < 2; pass++) {
		// counter, records and the ordering's scratch in ONE block of the call's own lease: the list comes back from the
		// scan in (stream, offset) order on the call's private stream -- nothing shared with other callers, no lock, no
		// allocation in steady state (round 3 ordered through btbbx_sort_hits_device's per-device scratch and its mutex)
		const size_t rec_bytes = ((size_t)dev_cap * sizeof(btbbx_hit) + 255) & ~(size_t)255;
		const size_t order_bytes = dev_cap >= 2 ? btbbx_scan_ordered_scratch_bytes(search_bits, 1, lap, dev_cap) : 0;   // (segment slots where the scan has them)
		char *block = (char *)scope_hits(256 + rec_bytes + order_bytes);
		if (!block)
			return BTBBX_E_NOMEM;
		d.count = (uint32_t *)block;
		d.hits = (btbbx_hit *)(block + 256);
		HIP_TRY(hipMemsetAsync(d.count, 0, sizeof(uint32_t), q));
		int rc = dev_cap >= 2 && search_bits
			? btbbx_scan_ordered_device(d_words, n_words, n_words, 1, search_bits, lap, max_ac_errors, d.hits, dev_cap, d.count,
						    block + 256 + rec_bytes, order_bytes, q)
			: btbbx_scan_device(d_words, n_words, n_words, 1, search_bits, lap, max_ac_errors, d.hits, dev_cap, d.count, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(&count, d.count, sizeof(count), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (count <= dev_cap || cap == 0)
			break;
		// more matches than records kept, and the kept ones are whichever lanes came first: repeat
		// with room for all of them, then keep the smallest
		dev_cap = count;
	}
	const uint32_t have = count < dev_cap ? count : dev_cap;
	if (have) {
		const uint64_t n = have < cap ? have : cap;
		HIP_TRY(hipMemcpyAsync(hits, d.hits, (size_t)n * sizeof(btbbx_hit), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (offset_base)
			for (uint64_t i = 0; i < n; i++)
				hits[i].offset += offset_base;
	}
	return (int64_t)count;
}

extern "C" int64_t btbbx_scan_host(const uint64_t *words, uint64_t n_words, uint64_t search_bits,
				   uint32_t lap, int max_ac_errors, btbbx_hit *hits, uint64_t cap)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	rc = check_scan_args("btbbx_scan", 64, n_words, n_words, 1, search_bits);
	if (rc)
		return rc;
	CallScope scope;
	hipStream_t q = scope_stream();
	uint64_t *d_words = (uint64_t *)scope_device((n_words + 2) * 8);
	if (!d_words)
		return BTBBX_E_NOMEM;
	HIP_TRY(hipMemcpyAsync(d_words, words, n_words * 8, hipMemcpyHostToDevice, q));
	return scan_resident(d_words, n_words, search_bits, lap, max_ac_errors, hits, cap, 0, q);
}

extern "C" int64_t btbbx_scan_symbols(const char *symbols, uint64_t n_symbols, uint64_t search_length,
				      uint32_t lap, int max_ac_errors, btbbx_hit *hits, uint64_t cap)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (search_length + 63 > n_symbols) {
		set_error("btbbx_scan_symbols: search_length + 63 exceeds n_symbols");
		return BTBBX_E_ARG;
	}
	CallScope scope;
	hipStream_t q = scope_stream();
	uint64_t n_words = (n_symbols + 63) / 64;
	size_t sym_bytes = (n_symbols + 15) & ~15ULL;
	char *block = (char *)scope_device(sym_bytes + (n_words + 2) * 8);
	if (!block)
		return BTBBX_E_NOMEM;
	uint8_t *d_sym = (uint8_t *)block;
	uint64_t *d_words = (uint64_t *)(block + sym_bytes);
	HIP_TRY(hipMemcpyAsync(d_sym, symbols, n_symbols, hipMemcpyHostToDevice, q));
	rc = btbbx_pack_device(d_sym, n_symbols, d_words, q);
	if (rc)
		return rc;
	return scan_resident(d_words, n_words, search_length, lap, max_ac_errors, hits, cap, 0, q);
}

// First match of one symbol-per-byte buffer (what btbb_find_ac returns, bluetooth_packet.c:444-464):
// one pinned staging copy in, pack + scan (atomicMin over offset << 32 | lap << 8 | errors) queued
// behind it, 8 bytes back, one synchronisation.
extern "C" int btbbx_find_first_symbols(const char *symbols, uint64_t n_symbols, uint64_t search_length,
					uint32_t lap, int max_ac_errors, btbbx_hit *first_hit)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!symbols || !first_hit || search_length + 63 > n_symbols || search_length >= (1ULL << 32)) {
		set_error("btbbx_find_first_symbols: bad argument (search_length + 63 must not exceed n_symbols, search_length < 2^32)");
		return BTBBX_E_ARG;
	}
	if (search_length == 0)
		return 0;
	CallScope scope;                                  // private scratch + stream: callers may be concurrent
	hipStream_t q = scope_stream();
	const uint64_t n_sym = search_length + 63;            // last symbol the reference reads
	const uint64_t n_words = (n_sym + 63) / 64;
	const size_t sym_bytes = (n_sym + 15) & ~15ULL;
	// Device block: symbols | sentinel for the first-match word | packed words.  The sentinel sits
	// right behind the symbols so that ONE host-to-device copy from pinned staging brings both in.
	char *block = (char *)scope_device(sym_bytes + (n_words + 2) * 8 + 16);
	char *stage = (char *)scope_pinned(sym_bytes + 16);
	if (!block || !stage)
		return BTBBX_E_NOMEM;
	uint8_t *d_sym = (uint8_t *)block;
	uint64_t *d_first = (uint64_t *)(block + sym_bytes);
	uint64_t *d_words = d_first + 1;
	uint64_t first = ~0ULL;
	memcpy(stage, symbols, n_sym);
	memcpy(stage + sym_bytes, &first, 8);
	HIP_TRY(hipMemcpyAsync(d_sym, stage, sym_bytes + 8, hipMemcpyHostToDevice, q));
	rc = btbbx_pack_device(d_sym, n_sym, d_words, q);
	if (!rc)
		rc = btbbx_scan_first_device(d_words, n_words, search_length, lap, max_ac_errors, d_first, q);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpyAsync(stage + sym_bytes + 8, d_first, 8, hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	memcpy(&first, stage + sym_bytes + 8, 8);
	if (first == ~0ULL)
		return 0;
	memset(first_hit, 0, sizeof(*first_hit));
	first_hit->offset = first >> 32;
	first_hit->lap = lap == BTBBX_LAP_ANY ? (uint32_t)(first >> 8) & 0xffffff : lap;
	first_hit->ac_errors = (uint8_t)(first & 0xff);
	return 1;
}

// ---- time sharding over the GPUs of one node -------------------------------------
//
// The path shards with no exchange step: shard k owns a contiguous, word-aligned range of offsets and
// reads 63 symbols past its end (an access code that starts at the last owned offset ends there).
// The same plan serves one-process-per-GPU callers (bench.py, torch.distributed ranks: each rank asks
// for its own shard) and btbbx_scan_host_multi below (one host thread per listed device).

extern "C" int btbbx_shard_plan(uint64_t search_bits, uint32_t n_shards, uint32_t shard, btbbx_shard *out)
{
	if (!out || n_shards == 0 || shard >= n_shards) {
		set_error("btbbx_shard_plan: shard %u of %u", shard, n_shards);
		return BTBBX_E_ARG;
	}
	const uint64_t words_total = (search_bits + 63) / 64;
	const uint64_t per = (words_total + n_shards - 1) / n_shards;
	uint64_t w0 = (uint64_t)shard * per;
	if (w0 > words_total)
		w0 = words_total;
	uint64_t w1 = w0 + per;
	if (w1 > words_total)
		w1 = words_total;
	uint64_t end = w1 * 64;
	if (end > search_bits)
		end = search_bits;
	out->first_word = w0;
	out->first_offset = w0 * 64;
	out->search_bits = end > w0 * 64 ? end - w0 * 64 : 0;
	out->n_words = out->search_bits ? (out->search_bits + 63 + 63) / 64 : 0;
	return BTBBX_OK;
}

extern "C" int64_t btbbx_scan_host_multi(const uint64_t *words, uint64_t n_words, uint64_t search_bits, uint32_t lap,
					 int max_ac_errors, btbbx_hit *hits, uint64_t cap, const int *devices,
					 int n_devices)
{
	if (!words || n_devices <= 0 || !devices || (!hits && cap)) {
		set_error("btbbx_scan_host_multi: bad argument");
		return BTBBX_E_ARG;
	}
	int rc = check_scan_args("btbbx_scan", 64, n_words, n_words, 1, search_bits);
	if (rc)
		return rc;
	struct Part {
		btbbx_shard plan;
		std::vector<btbbx_hit> hits;
		int64_t found = 0;
		char err[256] = "";
	};
	std::vector<Part> parts((size_t)n_devices);
	std::vector<std::thread> workers;
	int home = 0;
	(void)hipGetDevice(&home);
	for (int k = 0; k < n_devices; k++) {
		Part &p = parts[(size_t)k];
		btbbx_shard_plan(search_bits, (uint32_t)n_devices, (uint32_t)k, &p.plan);
		if (!p.plan.search_bits)
			continue;
		const int dev = devices[k];
		workers.emplace_back([&p, dev, words, lap, max_ac_errors, cap]() {
			auto fail = [&p](int64_t code) {
				p.found = code;
				snprintf(p.err, sizeof(p.err), "%s", btbbx_last_error());
			};
			if (hipSetDevice(dev) != hipSuccess)
				return fail(hip_fail(hipGetLastError(), "hipSetDevice"));
			int rc = ctx_require();
			if (rc)
				return fail(rc);
			CallScope scope;
			hipStream_t q = scope_stream();
			uint64_t *d_words = (uint64_t *)scope_device((p.plan.n_words + 2) * 8);
			if (!d_words)
				return fail(BTBBX_E_NOMEM);
			if (hipMemcpyAsync(d_words, words + p.plan.first_word, p.plan.n_words * 8, hipMemcpyHostToDevice, q) !=
			    hipSuccess)
				return fail(hip_fail(hipGetLastError(), "shard upload"));
			// a shard can hold at most what the caller takes in total
			uint64_t want = p.plan.search_bits / 256 + 4096;
			if (want > cap)
				want = cap;
			for (;;) {
				p.hits.resize((size_t)want);
				const int64_t n = scan_resident(d_words, p.plan.n_words, p.plan.search_bits, lap, max_ac_errors,
								p.hits.data(), want, p.plan.first_offset, q);
				if (n < 0)
					return fail(n);
				p.found = n;
				if ((uint64_t)n <= want || want >= cap)
					break;
				want = (uint64_t)n < cap ? (uint64_t)n : cap;      // dense stream: once more with room
			}
			p.hits.resize((size_t)((uint64_t)p.found < want ? (uint64_t)p.found : want));
		});
	}
	for (std::thread &t : workers)
		t.join();
	(void)hipSetDevice(home);
	int64_t total = 0;
	uint64_t written = 0;
	for (const Part &p : parts) {
		if (p.found < 0) {
			set_error("btbbx_scan_host_multi: %s", p.err);
			return p.found;
		}
		total += p.found;
		// shards are disjoint and ascending: concatenation is the (stream, offset) order
		for (size_t i = 0; i < p.hits.size() && written < cap; i++)
			hits[written++] = p.hits[i];
	}
	return total;
}
