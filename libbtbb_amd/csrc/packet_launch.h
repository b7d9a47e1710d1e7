// packet_launch.h -- the launchers of the packet chain that are not part of the exported ABI (defined in packet.hip; called
// from survey.hip and btbb_api.cpp).  d_count (may be null): the number of packets as a word in HBM, n_packets then being
// the capacity the launch is sized for.
#pragma once
#include "common.h"
#include "packet_obj.h"

int launch_gather(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, const btbbx_hit *d_hits, uint32_t n_packets,
		  const uint32_t *d_count, uint32_t max_length, uint64_t *d_packets, uint32_t *d_lengths, hipStream_t hip_stream);
int launch_trials(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets, const uint32_t *d_count,
		  btbbx_trial *d_trials, hipStream_t hip_stream);
int launch_header_flags(const uint64_t *d_packets, const uint32_t *d_lengths, uint32_t n_packets, const uint32_t *d_count,
			uint8_t *d_present, hipStream_t stream);
int launch_decode(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
		  btbbx_pkt_out *d_out, uint32_t mode, const TrialPlan *plan, hipStream_t stream);
// the drop-in API's single-packet calls (d_state: trials_state_bytes() bytes)
int launch_decode_bytes(const uint8_t *d_sym, uint8_t *d_pay, const btbbx_pkt_in *d_in, btbbx_pkt_out *d_out,
			uint32_t mode, bool with_payload, hipStream_t stream);
int launch_trials_state(const uint8_t *d_sym, const btbbx_pkt_in *d_in, const btbbx_pkt_out *d_out, void *d_state,
			btbbx_trial *d_trials, hipStream_t stream);
int launch_trials_merge(const void *d_state, const btbbx_pkt_in *d_in, btbbx_pkt_out *d_out, uint8_t *d_pay,
			const TrialPlan *plan, hipStream_t stream);
size_t trials_state_bytes();
