// hop.hip -- Bluetooth BR hop selection and CLK1-27 reversal on the GPU: the host side of it.
//
// Replaces lib/src/bluetooth_piconet.c:171-362 (precalc, address_precalc, perm5/fast_perm,
// gen_hops), :443-472 (hop, aliased_channel, init_candidates) and :575-645 (channel_winnow,
// btbb_winnow).  The reference materialises the whole 2^27-entry pattern (128 MiB, about a
// second of CPU per address) and then filters candidate clocks by table look-ups.  Here the
// selection kernel is a pure function evaluated where it is needed:
//   * hop_sequence_kernel   fills sequence[first .. first+count) for callers that want the
//                           table (one lane per 64 hops; the permutation is applied to a
//                           32-byte window of the bank table held in registers);
//   * candidates / winnow   evaluate the kernel per candidate clock -- no table at all.
// The kernels are in the headers below, one per family; this file is the host side.
#include <string.h>
#include <stdlib.h>
#include <mutex>
#include <vector>
#include "hop_core.h"
#include "hop_sequence.h"
#include "hop_reversal.h"
#include "hop_batch.h"

// hop selection needs a GPU but none of the btbb_init() tables
static int hop_device()
{
	if (ctx().ready)
		return BTBBX_OK;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
		set_error("hop: no usable HIP device");
		return BTBBX_E_NODEVICE;
	}
	return BTBBX_OK;
}

static bool hip_bad(hipError_t e, const char *what) { return e != hipSuccess && hip_fail(e, what) != 0; }

static int hop_args(const btbbx_hop_cfg *cfg, HopArgs *h)
{
	if (!cfg) {
		set_error("hop: NULL configuration");
		return BTBBX_E_ARG;
	}
	hop_address_fields(cfg->address, cfg->afh, cfg->used_channels, h);
	if (h->mod == 0 || h->mod > 80) {
		set_error("hop: AFH pattern with %u used channels", h->mod);
		return BTBBX_E_ARG;
	}
	memcpy(h->bank, cfg->bank, sizeof(h->bank));
	return BTBBX_OK;
}

// sub-allocation from one block: the offset of the next `bytes`, 256-byte aligned; off = the block's size so far
static size_t carve(size_t &off, size_t bytes)
{
	const size_t o = off;
	off += (bytes + 255) & ~(size_t)255;
	return o;
}

// Device and pinned buffers of one reversal; recycled through a small pool because a handle is
// opened per piconet and per restart (hipMalloc/hipHostMalloc cost far more than the kernels).
struct HopWorkspace {
	void *d_block;            // one allocation, carved below
	uint32_t *d_cand[2];      // ping-pong lists, HOP_GROUPS entries each
	uint64_t *d_masks;        // HOP_GROUPS / 64 words
	uint32_t *d_prefix;
	uint16_t *d_agree;
	uint32_t *d_hist;         // HOP_MAX_OBS + 1
	HopObs *d_obs;
	WinnowVerdict *d_verdict;
	uint32_t *d_total;
	int device;               // the HIP device the block lives on (a workspace is only reused there)
	void *h_block;            // pinned: observations going in, verdict / total coming back
	HopObs *h_obs;
	WinnowVerdict *h_verdict;
	uint32_t *h_total;
	hipStream_t stream;
};

static std::mutex pool_lock;
static std::vector<HopWorkspace *> pool;
#define HOP_POOL_MAX 8

static void workspace_free(HopWorkspace *w)
{
	if (!w)
		return;
	if (w->d_block)
		(void)hipFree(w->d_block);
	if (w->h_block)
		(void)hipHostFree(w->h_block);
	if (w->stream)
		(void)hipStreamDestroy(w->stream);
	free(w);
}

static HopWorkspace *workspace_get()
{
	int dev = 0;
	(void)hipGetDevice(&dev);
	{
		std::lock_guard<std::mutex> g(pool_lock);
		for (size_t i = 0; i < pool.size(); i++)
			if (pool[i]->device == dev) {
				HopWorkspace *w = pool[i];
				pool.erase(pool.begin() + (long)i);
				return w;
			}
	}
	HopWorkspace *w = (HopWorkspace *)calloc(1, sizeof(*w));
	if (!w)
		return nullptr;
	w->device = dev;
	size_t off = 0;
	const size_t o_c0 = carve(off, sizeof(uint32_t) * HOP_GROUPS), o_c1 = carve(off, sizeof(uint32_t) * HOP_GROUPS);
	const size_t o_m = carve(off, sizeof(uint64_t) * (HOP_GROUPS / 64)), o_p = carve(off, sizeof(uint32_t) * (HOP_GROUPS / 64));
	const size_t o_a = carve(off, sizeof(uint16_t) * HOP_GROUPS), o_h = carve(off, sizeof(uint32_t) * (HOP_MAX_OBS + 1));
	const size_t o_o = carve(off, sizeof(HopObs) * HOP_MAX_OBS), o_v = carve(off, sizeof(WinnowVerdict)), o_t = carve(off, sizeof(uint32_t));
	hipError_t e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
	if (e == hipSuccess)
		e = hipMalloc(&w->d_block, off);
	if (e == hipSuccess)
		e = hipHostMalloc(&w->h_block, sizeof(HopObs) * HOP_MAX_OBS + 256, hipHostMallocDefault);
	if (e != hipSuccess) {
		hip_fail(e, "hop workspace allocation");
		workspace_free(w);
		return nullptr;
	}
	char *d = (char *)w->d_block, *hp = (char *)w->h_block;
	w->d_cand[0] = (uint32_t *)(d + o_c0);
	w->d_cand[1] = (uint32_t *)(d + o_c1);
	w->d_masks = (uint64_t *)(d + o_m);
	w->d_prefix = (uint32_t *)(d + o_p);
	w->d_agree = (uint16_t *)(d + o_a);
	w->d_hist = (uint32_t *)(d + o_h);
	w->d_obs = (HopObs *)(d + o_o);
	w->d_verdict = (WinnowVerdict *)(d + o_v);
	w->d_total = (uint32_t *)(d + o_t);
	w->h_obs = (HopObs *)hp;
	w->h_verdict = (WinnowVerdict *)(hp + sizeof(HopObs) * HOP_MAX_OBS);
	w->h_total = (uint32_t *)(hp + sizeof(HopObs) * HOP_MAX_OBS + 64);
	return w;
}

void hop_pool_release()        // btbbx_shutdown
{
	std::lock_guard<std::mutex> g(pool_lock);
	for (HopWorkspace *w : pool)
		workspace_free(w);
	pool.clear();
}

static void workspace_put(HopWorkspace *w)
{
	if (!w)
		return;
	{
		std::lock_guard<std::mutex> g(pool_lock);
		if (pool.size() < HOP_POOL_MAX) {
			pool.push_back(w);
			return;
		}
	}
	workspace_free(w);
}

struct btbbx_hop_reversal {
	HopArgs h;
	int aliased;
	uint32_t n;               // candidates
	int cur;                  // which of the two lists is current
	HopWorkspace *w;
};

extern "C" {

void btbbx_hop_cfg_init(btbbx_hop_cfg *cfg, uint32_t address, const uint8_t *afh_map)
{
	memset(cfg, 0, sizeof(*cfg));
	cfg->address = address & 0xfffffff;
	int j = 0;
	for (int i = 0; i < HOP_NCHAN; i++) {                       // precalc, bluetooth_piconet.c:171-194
		const int chan = (2 * i) % HOP_NCHAN;
		if (!afh_map)
			cfg->bank[i] = (uint8_t)chan;
		else if (afh_map[chan / 8] & (1 << (chan % 8)))
			cfg->bank[j++] = (uint8_t)chan;
	}
	if (afh_map) {
		cfg->afh = 1;
		for (int i = 0; i < 10; i++)                        // btbb_piconet_set_afh_map, :122-131
			cfg->used_channels += (uint8_t)__builtin_popcount(afh_map[i]);
	} else {
		cfg->used_channels = HOP_NCHAN;
	}
}

int btbbx_hop_sequence_device(const btbbx_hop_cfg *cfg, uint64_t first, uint64_t count, uint8_t *d_sequence,
			      void *hip_stream)
{
	int rc = hop_device();
	if (rc)
		return rc;
	HopArgs h;
	if ((rc = hop_args(cfg, &h)))
		return rc;
	if ((first & 63) || (count & 63) || first + count > BTBBX_SEQUENCE_LENGTH || !d_sequence ||
	    ((uintptr_t)d_sequence & 15)) {
		set_error("hop_sequence: range [%llu, +%llu) must be 64-aligned inside 2^27, buffer 16-byte aligned",
			  (unsigned long long)first, (unsigned long long)count);
		return BTBBX_E_ARG;
	}
	if (!count)
		return BTBBX_OK;
	const uint32_t nt = (uint32_t)(count >> 6);
	hipLaunchKernelGGL(hop_sequence_kernel, dim3((nt + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, h,
			   (uint32_t)(first >> 6), nt, (uint4 *)d_sequence);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

int btbbx_hop_channels_device(const btbbx_hop_cfg *cfg, const uint32_t *d_clocks, uint32_t n, uint8_t *d_channels,
			      void *hip_stream)
{
	int rc = hop_device();
	if (rc)
		return rc;
	HopArgs h;
	if ((rc = hop_args(cfg, &h)))
		return rc;
	if (!n)
		return BTBBX_OK;
	hipLaunchKernelGGL(hop_channels_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, h, d_clocks, n,
			   d_channels);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

void btbbx_hop_reversal_close(btbbx_hop_reversal *r)
{
	if (!r)
		return;
	workspace_put(r->w);
	free(r);
}

static int reversal_compact(btbbx_hop_reversal *r, uint32_t nwords, const uint32_t *src, uint32_t base, uint32_t *dst)
{
	HopWorkspace *w = r->w;
	hipLaunchKernelGGL(hop_mask_prefix_kernel, dim3(1), dim3(1024), 0, w->stream, w->d_masks, nwords, w->d_prefix,
			   w->d_total);
	hipLaunchKernelGGL(hop_scatter_kernel, dim3((nwords + 255) / 256), dim3(256), 0, w->stream, w->d_masks, w->d_prefix,
			   nwords, src, base, dst);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

btbbx_hop_reversal *btbbx_hop_reversal_open(const btbbx_hop_cfg *cfg, uint32_t clk6, uint8_t channel, int aliased,
					    int *n_candidates)
{
	if (hop_device())
		return nullptr;
	btbbx_hop_reversal *r = (btbbx_hop_reversal *)calloc(1, sizeof(*r));
	if (!r || hop_args(cfg, &r->h) || !(r->w = workspace_get())) {
		free(r);
		return nullptr;
	}
	HopWorkspace *w = r->w;
	r->aliased = aliased != 0;
	hipLaunchKernelGGL(hop_candidate_mask_kernel, dim3(HOP_GROUPS / 256), dim3(256), 0, w->stream, r->h, clk6 & 63u,
			   (int)(int8_t)channel, r->aliased, w->d_masks);
	if (reversal_compact(r, HOP_GROUPS / 64, nullptr, clk6 & 63u, w->d_cand[0]) ||
	    hip_bad(hipMemcpyAsync(w->h_total, w->d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream), "copy") ||
	    hip_bad(hipStreamSynchronize(w->stream), "hop_reversal_open")) {
		btbbx_hop_reversal_close(r);
		return nullptr;
	}
	r->n = *w->h_total;
	r->cur = 0;
	if (n_candidates)
		*n_candidates = (int)r->n;
	return r;
}

int btbbx_hop_reversal_winnow(btbbx_hop_reversal *r, const int32_t *index_offsets, const uint8_t *channels,
			      uint32_t n_obs, uint32_t *stop, uint32_t *count, uint32_t *cand0)
{
	if (!r || (n_obs && (!index_offsets || !channels)) || n_obs > HOP_MAX_OBS) {
		set_error("hop_reversal_winnow: bad arguments (n_obs %u)", n_obs);
		return BTBBX_E_ARG;
	}
	HopWorkspace *w = r->w;
	WinnowVerdict v = {n_obs, r->n, 0, 0};
	if (n_obs && r->n) {
		for (uint32_t k = 0; k < n_obs; k++) {
			w->h_obs[k].offset = index_offsets[k];
			w->h_obs[k].channel = (int)(int8_t)channels[k];
		}
		const uint32_t n = r->n, nwords = (n + 63) / 64;
		uint32_t *src = w->d_cand[r->cur], *dst = w->d_cand[r->cur ^ 1];
		HIP_TRY(hipMemcpyAsync(w->d_obs, w->h_obs, sizeof(HopObs) * n_obs, hipMemcpyHostToDevice, w->stream));
		if (n <= HOP_SMALL_N) {
			hipLaunchKernelGGL(hop_winnow_small_kernel, dim3(1), dim3(1024), 0, w->stream, r->h, src, n, w->d_obs,
					   n_obs, r->aliased, dst, w->d_verdict);
		} else {
			HIP_TRY(hipMemsetAsync(w->d_hist, 0, sizeof(uint32_t) * (n_obs + 1), w->stream));
			hipLaunchKernelGGL(hop_winnow_kernel, dim3((n + 255) / 256), dim3(256), 0, w->stream, r->h, src, n,
					   w->d_obs, n_obs, r->aliased, w->d_agree, w->d_hist);
			hipLaunchKernelGGL(hop_verdict_kernel, dim3(1), dim3(1024), 0, w->stream, w->d_hist, n, n_obs,
					   w->d_verdict);
			hipLaunchKernelGGL(hop_agree_mask_kernel, dim3((nwords * 64 + 255) / 256), dim3(256), 0, w->stream,
					   w->d_agree, n, w->d_verdict, w->d_masks);
			int rc = reversal_compact(r, nwords, src, 0, dst);
			if (rc)
				return rc;
		}
		hipLaunchKernelGGL(hop_first_kernel, dim3(1), dim3(1), 0, w->stream, dst, w->d_verdict);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(w->h_verdict, w->d_verdict, sizeof(v), hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
		v = *w->h_verdict;
		r->cur ^= 1;
		r->n = v.count;
	} else if (n_obs) {
		// An empty list (channel never produced by this pattern, e.g. >= 79 or outside the AFH bank):
		// the reference's channel_winnow still runs for the first unused observation, finds no
		// candidate and resets the piconet (bluetooth_piconet.c:596-601, 614-620) -- so the walk
		// stops at observation 0 with nothing left.
		v.stop = 0;
		v.count = 0;
	} else if (r->n) {
		HIP_TRY(hipMemcpyAsync(w->h_total, w->d_cand[r->cur], sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
		v.cand0 = *w->h_total;
	}
	if (stop) *stop = v.stop;
	if (count) *count = v.count;
	if (cand0) *cand0 = v.cand0;
	return BTBBX_OK;
}

int64_t btbbx_hop_reversal_candidates(btbbx_hop_reversal *r, uint32_t *dst, uint64_t cap)
{
	if (!r)
		return BTBBX_E_ARG;
	const uint64_t k = r->n < cap ? r->n : cap;
	if (k && dst) {
		HIP_TRY(hipMemcpyAsync(dst, r->w->d_cand[r->cur], k * sizeof(uint32_t), hipMemcpyDeviceToHost, r->w->stream));
		HIP_TRY(hipStreamSynchronize(r->w->stream));
	}
	return (int64_t)r->n;
}


// rows + thresholds; the same for every cand_cap (no candidate is ever stored outside the caller's d_candidates)
size_t btbbx_hop_reversal_batch_scratch_bytes(uint32_t job_cap, uint32_t cand_cap)
{
	(void)cand_cap;
	const size_t bytes = (size_t)job_cap * (2 * HOP_BINS + 1) * sizeof(uint32_t);
	return (bytes + 255) & ~(size_t)255;
}

int btbbx_hop_reversal_batch_device(const btbbx_clock_job *d_jobs, const uint32_t *d_n_jobs, uint32_t job_cap,
				    const int32_t *d_index_offsets, const uint8_t *d_channels, uint32_t n_obs_total,
				    btbbx_clock_result *d_results, uint32_t *d_candidates, uint32_t cand_cap,
				    void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const size_t need = btbbx_hop_reversal_batch_scratch_bytes(job_cap, cand_cap);
	if (!d_jobs || !d_results || !d_scratch || !job_cap || job_cap > 0x7fffffffu || scratch_bytes < need ||
	    (n_obs_total && (!d_index_offsets || !d_channels))) {
		set_error("btbbx_hop_reversal_batch_device: null pointer, no jobs (or 2^31 and more), or scratch of %zu bytes needed and "
			  "%zu given", need, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_jobs & 3) || ((uintptr_t)d_n_jobs & 3) || ((uintptr_t)d_index_offsets & 3) || ((uintptr_t)d_results & 3) ||
	    ((uintptr_t)d_candidates & 3) || ((uintptr_t)d_scratch & 15)) {
		set_error("btbbx_hop_reversal_batch_device: misaligned pointer (scratch 16 bytes, everything else but the channels 4)");
		return BTBBX_E_ARG;
	}
	int rc = hop_device();
	if (rc)
		return rc;
	hipStream_t q = (hipStream_t)hip_stream;
	uint32_t *rows = (uint32_t *)d_scratch, *keep = rows + (size_t)job_cap * 2 * HOP_BINS;
	// tiles per job: enough workgroups for the device from a few jobs, long tiles (the table and the observations are
	// staged once per workgroup) from many
	uint32_t tiles_log2 = 9;
	while (tiles_log2 > 4 && ((uint64_t)job_cap << tiles_log2) > 16384)
		tiles_log2--;
	while (tiles_log2 && ((uint64_t)job_cap << tiles_log2) > 0x7fffffffu)
		tiles_log2--;
	HIP_TRY(hipMemsetAsync(rows, 0, (size_t)job_cap * 2 * HOP_BINS * sizeof(uint32_t), q));
	hipLaunchKernelGGL(hop_batch_agree_kernel, dim3(job_cap << tiles_log2), dim3(256), 0, q, d_jobs, d_n_jobs, job_cap, tiles_log2,
			   d_index_offsets, d_channels, n_obs_total, rows);
	hipLaunchKernelGGL(hop_batch_verdict_kernel, dim3(job_cap), dim3(1024), 0, q, d_jobs, d_n_jobs, job_cap, n_obs_total, rows, keep,
			   d_results, d_candidates, cand_cap);
	if (d_candidates && cand_cap)
		hipLaunchKernelGGL(hop_batch_emit_kernel, dim3(job_cap), dim3(1024), 0, q, d_jobs, d_n_jobs, job_cap, d_index_offsets,
				   d_channels, keep, d_results, d_candidates, cand_cap);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

int64_t btbbx_hop_reversal_batch_host(const btbbx_clock_job *jobs, uint32_t n_jobs, const int32_t *index_offsets,
				      const uint8_t *channels, uint32_t n_obs_total, btbbx_clock_result *results,
				      uint32_t *candidates, uint32_t cand_cap)
{
	if ((n_jobs && (!jobs || !results)) || n_jobs > 0x7fffffffu || (n_obs_total && (!index_offsets || !channels))) {
		set_error("btbbx_hop_reversal_batch_host: null pointer or 2^31 jobs and more");
		return BTBBX_E_ARG;
	}
	int rc = hop_device();
	if (rc)
		return rc;
	if (!n_jobs)
		return 0;
	// one device block and one stream per call: concurrent callers share nothing
	size_t off = 0;
	const size_t want_cand = candidates ? (size_t)n_jobs * cand_cap * sizeof(uint32_t) : 0;
	const size_t scratch_bytes = btbbx_hop_reversal_batch_scratch_bytes(n_jobs, cand_cap);
	const size_t o_scr = carve(off, scratch_bytes), o_jobs = carve(off, (size_t)n_jobs * sizeof(*jobs));
	const size_t o_res = carve(off, (size_t)n_jobs * sizeof(*results)), o_off = carve(off, (size_t)n_obs_total * sizeof(int32_t));
	const size_t o_ch = carve(off, n_obs_total), o_cand = carve(off, want_cand);
	char *d = nullptr;
	hipStream_t q = nullptr;
	if (hipMalloc((void **)&d, off) != hipSuccess) {
		(void)hipGetLastError();
		set_error("btbbx_hop_reversal_batch_host: %zu bytes of device memory for %u jobs not available", off, n_jobs);
		return BTBBX_E_NOMEM;
	}
	hipError_t e = hipStreamCreateWithFlags(&q, hipStreamNonBlocking);
	if (e == hipSuccess)
		e = hipMemcpyAsync(d + o_jobs, jobs, (size_t)n_jobs * sizeof(*jobs), hipMemcpyHostToDevice, q);
	if (e == hipSuccess && n_obs_total)
		e = hipMemcpyAsync(d + o_off, index_offsets, (size_t)n_obs_total * sizeof(int32_t), hipMemcpyHostToDevice, q);
	if (e == hipSuccess && n_obs_total)
		e = hipMemcpyAsync(d + o_ch, channels, n_obs_total, hipMemcpyHostToDevice, q);
	// the caller's candidate slots go in first, so that the slots no job writes come back as they were
	if (e == hipSuccess && want_cand)
		e = hipMemcpyAsync(d + o_cand, candidates, want_cand, hipMemcpyHostToDevice, q);
	if (e == hipSuccess) {
		rc = btbbx_hop_reversal_batch_device((const btbbx_clock_job *)(d + o_jobs), nullptr, n_jobs, (const int32_t *)(d + o_off),
						     (const uint8_t *)(d + o_ch), n_obs_total, (btbbx_clock_result *)(d + o_res),
						     want_cand ? (uint32_t *)(d + o_cand) : nullptr, cand_cap, d + o_scr, scratch_bytes, q);
		if (!rc)
			e = hipMemcpyAsync(results, d + o_res, (size_t)n_jobs * sizeof(*results), hipMemcpyDeviceToHost, q);
		if (!rc && e == hipSuccess && want_cand)
			e = hipMemcpyAsync(candidates, d + o_cand, want_cand, hipMemcpyDeviceToHost, q);
	}
	const hipError_t f = q ? hipStreamSynchronize(q) : hipSuccess;
	if (q)
		(void)hipStreamDestroy(q);
	(void)hipFree(d);
	if (rc)
		return rc;
	HIP_TRY(e);
	HIP_TRY(f);
	return (int64_t)n_jobs;
}

} // extern "C"
