"""libbtbb_amd -- host-side Python view of the MI355X-native Bluetooth baseband scanner.

The product is the C-ABI shared library ``libbtbb_amd/libbtbb_amd.so`` (SONAME
``libbtbb.so.1``; sources in ``libbtbb_amd/csrc``, headers in ``include/``): a drop-in for the
baseband hot path of libbtbb whose computation runs in hand-written gfx950 HIP kernels.
This package only *binds* it with ctypes for the tests and the benchmark -- there is no
Python or CPU implementation of the path here, and loading fails loudly if the library has
not been built (``python -c "import __graft_entry__ as g; g.build()"``).

PyTorch (when present) is imported *before* the library so that both share one HIP runtime
(torch bundles its own libamdhip64.so); torch tensors' ``data_ptr()`` can then be handed to
the ``btbbx_*_device`` entry points.
"""
import ctypes as C
import os

import numpy as np

try:  # share torch's HIP runtime when torch is around (plumbing only)
    import torch as _torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the C library
    _torch = None

from . import synth  # noqa: F401  (host-side synthetic traffic, numpy)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LIBBTBB_AMD_SO") or os.path.join(_HERE, "libbtbb_amd.so")   # the override is for kernel A/B runs

LAP_ANY = 0xFFFFFFFF
PKT_WORDS = 50
MAX_SYMBOLS = 3125

# flag numbers (include/btbb.h)
BTBB_WHITENED, BTBB_NAP_VALID, BTBB_UAP_VALID, BTBB_LAP_VALID = 0, 1, 2, 3
BTBB_CLK6_VALID, BTBB_CLK27_VALID, BTBB_CRC_CORRECT, BTBB_HAS_PAYLOAD = 4, 5, 6, 7
BTBB_GOT_FIRST_PACKET, BTBB_FOLLOWING = 10, 14


class Hit(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("lap", C.c_uint32), ("ac_errors", C.c_uint8),
                ("reserved", C.c_uint8), ("stream", C.c_uint16)]


class Shard(C.Structure):
    _fields_ = [("first_word", C.c_uint64), ("n_words", C.c_uint64), ("search_bits", C.c_uint64),
                ("first_offset", C.c_uint64)]


class Trial(C.Structure):
    _fields_ = [("uap", C.c_uint8), ("type", C.c_uint8), ("rv", C.c_int16)]


class PktIn(C.Structure):
    _fields_ = [("length", C.c_uint32), ("clkn", C.c_uint32), ("flags", C.c_uint32),
                ("uap", C.c_uint8), ("type", C.c_uint8), ("llid", C.c_uint8), ("flow", C.c_uint8)]


class PktOut(C.Structure):
    _fields_ = [("header_rv", C.c_int32), ("payload_rv", C.c_int32), ("payload_length", C.c_int32),
                ("payload_header_length", C.c_int32), ("flags", C.c_uint32), ("header_packed", C.c_uint32),
                ("header_present", C.c_uint8), ("type", C.c_uint8), ("lt_addr", C.c_uint8),
                ("hdr_flags", C.c_uint8), ("hec", C.c_uint8), ("llid", C.c_uint8), ("flow", C.c_uint8),
                ("uap", C.c_uint8), ("payload_header", C.c_uint64), ("payload", C.c_uint64 * 43)]


HIT_DTYPE = np.dtype([("offset", "<u8"), ("lap", "<u4"), ("ac_errors", "u1"), ("reserved", "u1"), ("stream", "<u2")])
TRIAL_DTYPE = np.dtype([("uap", "u1"), ("type", "u1"), ("rv", "<i2")])
PKTIN_DTYPE = np.dtype([("length", "<u4"), ("clkn", "<u4"), ("flags", "<u4"), ("uap", "u1"), ("type", "u1"),
                        ("llid", "u1"), ("flow", "u1")])
PKTOUT_DTYPE = np.dtype([("header_rv", "<i4"), ("payload_rv", "<i4"), ("payload_length", "<i4"),
                         ("payload_header_length", "<i4"), ("flags", "<u4"), ("header_packed", "<u4"),
                         ("header_present", "u1"), ("type", "u1"), ("lt_addr", "u1"), ("hdr_flags", "u1"),
                         ("hec", "u1"), ("llid", "u1"), ("flow", "u1"), ("uap", "u1"),
                         ("payload_header", "<u8"), ("payload", "<u8", (43,))])
assert HIT_DTYPE.itemsize == C.sizeof(Hit) == 16
assert TRIAL_DTYPE.itemsize == C.sizeof(Trial) == 4
assert PKTIN_DTYPE.itemsize == C.sizeof(PktIn) == 16
assert PKTOUT_DTYPE.itemsize == C.sizeof(PktOut)

# Bluetooth LE (include/btbbx.h btbbx_le_*; le.hip checks the C layout with static_asserts)
LE_ADV_AA = 0x8E89BED6
LE_ADV_CRC_INIT = 0x555555
LE_MAX_BYTES = 64
LE_PKT_DTYPE = np.dtype([("offset", "<u8"), ("stream", "<u2"), ("aa_errors", "u1"), ("crc_ok", "u1"),
                         ("crc_rx", "<u4"), ("crc_calc", "<u4"), ("pdu_bytes", "<u2"), ("truncated", "u1"),
                         ("channel_idx", "u1"), ("channel_k", "u1"), ("is_data", "u1"), ("length", "u1"),
                         ("adv_type", "u1"), ("adv_tx_add", "u1"), ("adv_rx_add", "u1"), ("access_address_ok", "u1"),
                         ("access_address_offenses", "u1"), ("access_address", "<u4"), ("bytes", "u1", (LE_MAX_BYTES,)),
                         ("pad", "u1", (4,))])
assert LE_PKT_DTYPE.itemsize == 104 and LE_PKT_DTYPE.fields["bytes"][1] == 36

# LE Coded PHY (include/btbbx.h btbbx_le_coded_*; le_coded.h checks the C layout with a static_assert)
LE_CODED_PATTERN = 336
LE_CODED_MAX_ERRORS = 63
LE_CODED_LAG = 24
LE_CODED_INFO_DTYPE = np.dtype([("symbols", "<u4"), ("metric2", "<u4"), ("metric1", "<u2"), ("ci", "u1"), ("s", "u1"),
                                ("header_moved", "u1"), ("reserved", "u1", (3,))])
assert LE_CODED_INFO_DTYPE.itemsize == 16
# promiscuous LE Coded connection discovery (include/btbbx.h btbbx_le_cfind_*; le_cfind.h checks the C layout with a static_assert)
LE_CODED_CAND_INFO_DTYPE = np.dtype([("symbols", "<u4"), ("metric2", "<u4"), ("metric1", "<u2"), ("errors", "u1"), ("ci", "u1"),
                                     ("s", "u1"), ("reserved", "u1", (3,))])
assert LE_CODED_CAND_INFO_DTYPE.itemsize == 16

# LE connection discovery (include/btbbx.h btbbx_le_cand / btbbx_le_conn; le_discover.h checks the C layout with static_asserts)
LE_CAND_DTYPE = np.dtype([("offset", "<u8"), ("access_address", "<u4"), ("crc_init", "<u4"), ("stream", "<u2"),
                          ("header0", "u1"), ("length", "u1"), ("conn", "<u4")])
LE_CONN_DTYPE = np.dtype([("access_address", "<u4"), ("crc_init", "<u4"), ("n_packets", "<u4"), ("n_empty", "<u4"),
                          ("channel_mask", "<u8"), ("first", "<u8")])
LE_NO_CONN = 0xFFFFFFFF
assert LE_CAND_DTYPE.itemsize == 24 and LE_CONN_DTYPE.itemsize == 32
# LE connection tracking (include/btbbx.h btbbx_le_track / btbbx_le_track_pkt; le_track.h checks the C layout with static_asserts)
LE_TRACK_REMAP, LE_TRACK_TIMED, LE_TRACK_HOPPING = 1, 1, 2
LE_TRACK_DTYPE = np.dtype([("first_anchor", "<u8"), ("map_mask", "<u8"), ("n_events", "<u4"), ("n_fit", "<u4"), ("interval", "<u4"),
                           ("n_on_hop", "<u4"), ("n_off_hop", "<u4"), ("n_second", "<u4"), ("hop_increment", "u1"),
                           ("first_unmapped", "u1"), ("n_used", "u1"), ("flags", "u1"), ("reserved", "<u4")])
LE_TRACK_PKT_DTYPE = np.dtype([("rank", "<u4"), ("event", "<u4"), ("counter", "<u4"), ("channel", "u1"), ("unmapped", "u1"),
                               ("expected", "u1"), ("on_hop", "u1")])
assert LE_TRACK_DTYPE.itemsize == 48 and LE_TRACK_PKT_DTYPE.itemsize == 16
# LE channel selection #2 (include/btbbx.h btbbx_le_csa2 / btbbx_le_csa2_pkt; le_csa2.h checks the C layout with static_asserts)
LE_CSA2_REMAP, LE_CSA2_EVALUATED, LE_CSA2_UNIQUE, LE_CSA2_PREFERRED = 1, 1, 2, 4
LE_CSA2_DTYPE = np.dtype([("n_on", "<u4"), ("n_off", "<u4"), ("n_second", "<u4"), ("channel_id", "<u2"), ("counter0", "<u2"),
                          ("flags", "<u4"), ("reserved", "<u4")])
LE_CSA2_PKT_DTYPE = np.dtype([("counter", "<u2"), ("prn", "<u2"), ("unmapped", "u1"), ("expected", "u1"), ("on_hop", "u1"),
                              ("reserved", "u1")])
assert LE_CSA2_DTYPE.itemsize == 24 and LE_CSA2_PKT_DTYPE.itemsize == 8
# LE following from CONNECT_IND (include/btbbx.h btbbx_le_seed / btbbx_le_follow / btbbx_le_follow_pkt; le_follow.h checks the C
# layout with static_asserts)
LE_SEED_SEEDED = 1
LE_FOLLOW_SEEDED, LE_FOLLOW_COUNTED, LE_FOLLOW_STOPPED, LE_FOLLOW_TERMINATED, LE_FOLLOW_ENCRYPTED = 1, 2, 4, 8, 16
LE_STATE_COUNTED, LE_STATE_BEFORE, LE_STATE_BEYOND = 0, 1, 2
(LE_PDU_DATA, LE_PDU_CONTROL, LE_PDU_MAP_UPDATE, LE_PDU_PARAM_UPDATE, LE_PDU_TERMINATE, LE_PDU_ENC_START,
 LE_PDU_OPAQUE) = range(7)
LE_SEED_DTYPE = np.dtype([("t0", "<u8"), ("map", "<u8"), ("access_address", "<u4"), ("crc_init", "<u4"), ("request", "<u4"),
                          ("interval", "<u2"), ("win_offset", "<u2"), ("latency", "<u2"), ("timeout", "<u2"), ("win_size", "u1"),
                          ("hop", "u1"), ("sca", "u1"), ("chsel", "u1"), ("init_a", "u1", (6,)), ("adv_a", "u1", (6,)),
                          ("tx_add", "u1"), ("rx_add", "u1"), ("flags", "u1"), ("reserved", "u1")])
LE_FOLLOW_DTYPE = np.dtype([("map", "<u8"), ("counter_first", "<u4"), ("stop", "<u4"), ("n_before", "<u4"), ("n_on", "<u4"),
                            ("n_off", "<u4"), ("n_beyond", "<u4"), ("n_control", "<u4"), ("n_map_updates", "<u4"),
                            ("algorithm", "u1"), ("flags", "u1"), ("reserved", "u1", (6,))])
LE_FOLLOW_PKT_DTYPE = np.dtype([("counter", "<u4"), ("epoch", "<u2"), ("kind", "u1"), ("opcode", "u1"), ("expected", "u1"),
                                ("on_hop", "u1"), ("state", "u1"), ("reserved", "u1")])
assert LE_SEED_DTYPE.itemsize == 56 and LE_FOLLOW_DTYPE.itemsize == 48 and LE_FOLLOW_PKT_DTYPE.itemsize == 12
# LE following through connection parameter updates (include/btbbx.h btbbx_le_span / btbbx_le_span_pkt / btbbx_le_span_rec; le_span.h
# checks the C layout with static_asserts); the flags and states stand beside the LE_FOLLOW_* / LE_STATE_* values
LE_SPAN_CAPPED, LE_SPAN_REFUSED = 32, 64
LE_FOLLOW_DECRYPTED = 128       # btbbx_le_follow.flags and btbbx_le_span.flags, set by the keyed entries alone
LE_STATE_GAP = 3
LE_SPAN_DTYPE = np.dtype([("map", "<u8"), ("counter_first", "<u4"), ("stop", "<u4"), ("n_before", "<u4"), ("n_on", "<u4"),
                          ("n_off", "<u4"), ("n_beyond", "<u4"), ("n_gap", "<u4"), ("n_control", "<u4"), ("n_map_updates", "<u4"),
                          ("n_param_updates", "<u4"), ("n_spans", "<u4"), ("interval", "<u2"), ("algorithm", "u1"), ("flags", "u1")])
LE_SPAN_PKT_DTYPE = np.dtype([("counter", "<u4"), ("epoch", "<u2"), ("span", "<u2"), ("kind", "u1"), ("opcode", "u1"),
                              ("expected", "u1"), ("on_hop", "u1"), ("state", "u1"), ("applied", "u1"), ("reserved", "u1", (2,))])
LE_SPAN_REC_DTYPE = np.dtype([("origin", "<u8"), ("base", "<u4"), ("first_event", "<u4"), ("n_events", "<u4"), ("pdu", "<u4"),
                              ("interval", "<u2"), ("win_offset", "<u2"), ("latency", "<u2"), ("timeout", "<u2"), ("win_size", "u1"),
                              ("flags", "u1"), ("reserved", "u1", (6,))])
assert LE_SPAN_DTYPE.itemsize == 56 and LE_SPAN_PKT_DTYPE.itemsize == 16 and LE_SPAN_REC_DTYPE.itemsize == 40
# LE data extraction (include/btbbx.h btbbx_le_data / btbbx_le_data_pkt / btbbx_le_msg; le_data.h checks the C layout with
# static_asserts): a packet's kind, its sender's role, a message's flags
(LE_DATA_START, LE_DATA_CONTINUATION, LE_DATA_ORPHAN, LE_DATA_EMPTY, LE_DATA_CONTROL, LE_DATA_IGNORED, LE_DATA_RETRANSMIT,
 LE_DATA_UNKNOWN) = range(8)
LE_ROLE_CENTRAL, LE_ROLE_PERIPHERAL, LE_ROLE_UNKNOWN = 0, 1, 2
LE_MSG_COMPLETE, LE_MSG_OVERRUN, LE_MSG_RUNT, LE_MSG_STORED = 1, 2, 4, 8
LE_DATA_DTYPE = np.dtype([("bytes", "<u8"), ("first_msg", "<u4"), ("n_msgs", "<u4"), ("n_complete", "<u4"), ("n_central", "<u4"),
                          ("n_peripheral", "<u4"), ("n_unknown", "<u4"), ("n_retransmit", "<u4"), ("n_orphan", "<u4"),
                          ("n_control", "<u4"), ("n_empty", "<u4")])
LE_DATA_PKT_DTYPE = np.dtype([("msg", "<u4"), ("pos", "<u4"), ("role", "u1"), ("kind", "u1"), ("bits", "u1"), ("reserved", "u1")])
LE_MSG_DTYPE = np.dtype([("byte_offset", "<u8"), ("conn", "<u4"), ("start", "<u4"), ("n_fragments", "<u4"), ("bytes", "<u4"),
                         ("l2cap_len", "<u2"), ("cid", "<u2"), ("role", "u1"), ("flags", "u1"), ("reserved", "u1", (2,))])
assert LE_DATA_DTYPE.itemsize == 48 and LE_DATA_PKT_DTYPE.itemsize == 12 and LE_MSG_DTYPE.itemsize == 32
# LE decryption (include/btbbx.h btbbx_le_crypt / btbbx_le_crypt_pkt; le_crypt.h checks the C layout with static_asserts): a
# packet's state, a connection's flags
LE_CRYPT_CLEAR, LE_CRYPT_VERIFIED, LE_CRYPT_FAILED, LE_CRYPT_SKIPPED, LE_CRYPT_SHORT = range(5)
LE_CRYPT_REQ, LE_CRYPT_RSP, LE_CRYPT_START, LE_CRYPT_ARMED, LE_CRYPT_KEYED = 1, 2, 4, 8, 16
LE_CRYPT_DTYPE = np.dtype([("session_key", "u1", (16,)), ("iv", "u1", (8,)), ("req", "<u4"), ("rsp", "<u4"), ("start", "<u4"),
                           ("n_encrypted", "<u4"), ("n_verified", "<u4"), ("n_failed", "<u4"), ("n_skipped", "<u4"), ("key", "u1"),
                           ("max_skew", "u1"), ("flags", "u1"), ("reserved", "u1")])
LE_CRYPT_PKT_DTYPE = np.dtype([("counter", "<u4"), ("ordinal", "<u4"), ("state", "u1"), ("skew", "u1"), ("opcode", "u1"),
                               ("counter_hi", "u1"), ("reserved", "u1", (4,))])
assert LE_CRYPT_DTYPE.itemsize == 56 and LE_CRYPT_PKT_DTYPE.itemsize == 16
# LE legacy pairing key recovery (include/btbbx.h btbbx_le_pair; le_pair.h checks the C layout with a static_assert): a
# connection's pairing method, what of the exchange was found, which keys its record holds
LE_PAIR_NONE, LE_PAIR_LEGACY, LE_PAIR_SECURE, LE_PAIR_OOB, LE_PAIR_INVALID = range(5)
(LE_PAIR_PREQ, LE_PAIR_PRSP, LE_PAIR_MCONF, LE_PAIR_SCONF, LE_PAIR_MRAND, LE_PAIR_SRAND, LE_PAIR_ARMED,
 LE_PAIR_CRACKED) = 1, 2, 4, 8, 16, 32, 64, 128
LE_PAIR_KEY_STK, LE_PAIR_KEY_LTK_CENTRAL, LE_PAIR_KEY_LTK_PERIPHERAL = 1, 2, 4
LE_PAIR_MAX_TK, LE_PAIR_MAX_KEYS = 1000000, 64
LE_PAIR_DTYPE = np.dtype([("stk", "u1", (16,)), ("ltk", "u1", (2, 16)), ("preq", "<u4"), ("prsp", "<u4"), ("mconf", "<u4"),
                          ("sconf", "<u4"), ("mrand", "<u4"), ("srand", "<u4"), ("tk", "<u4"), ("method", "u1"), ("flags", "u1"),
                          ("keys", "u1"), ("key_size", "u1"), ("key", "u1"), ("reserved", "u1", (7,))])
assert LE_PAIR_DTYPE.itemsize == 88
# LE address resolution (include/btbbx.h btbbx_le_addr / btbbx_le_irk / btbbx_le_peer; le_resolve.h checks the C layout with
# static_asserts): an address's kind, the roles it was seen in, a table slot's flags
LE_ADDR_PUBLIC, LE_ADDR_NONRESOLVABLE, LE_ADDR_RESOLVABLE, LE_ADDR_RESERVED, LE_ADDR_STATIC = range(5)
LE_ADDR_ADVERTISER, LE_ADDR_SCANNER, LE_ADDR_INITIATOR, LE_ADDR_TARGET = 1, 2, 4, 8
LE_IRK_GIVEN, LE_IRK_HARVESTED, LE_IRK_HAS_ADDR, LE_IRK_NULLKEY = 1, 2, 4, 8
LE_RESOLVE_MAX_IRKS = 4096
LE_NO_ADDR, LE_NO_IRK = 0xFFFFFFFF, 0xFFFF
LE_ADDR_DTYPE = np.dtype([("first_offset", "<u8"), ("last_offset", "<u8"), ("n_slots", "<u4"), ("first_rec", "<u4"), ("addr", "u1", (6,)),
                          ("random", "u1"), ("kind", "u1"), ("irk", "<u2"), ("roles", "u1"), ("channels", "u1"), ("reserved", "u1", (4,))])
LE_IRK_DTYPE = np.dtype([("key", "u1", (16,)), ("id_addr", "u1", (6,)), ("id_random", "u1"), ("flags", "u1"), ("conn", "<u4"),
                         ("n_addrs", "<u4"), ("n_slots", "<u4"), ("role", "u1"), ("reserved", "u1", (3,))])
LE_PEER_DTYPE = np.dtype([("init_addr", "<u4"), ("adv_addr", "<u4"), ("init_irk", "<u2"), ("adv_irk", "<u2"), ("irk", "<u2", (2,))])
assert LE_ADDR_DTYPE.itemsize == 40 and LE_IRK_DTYPE.itemsize == 40 and LE_PEER_DTYPE.itemsize == 16

# one surveyed piconet (include/btbbx.h btbbx_survey_rec; survey.hip checks the C layout with static_asserts)
SURVEY_DTYPE = np.dtype([("lap", "<u4"), ("flags", "<u4"), ("uap", "u1"), ("clk_offset", "u1"), ("used_channels", "u1"),
                         ("settled_by", "u1"), ("afh_map", "u1", (10,)), ("first_stream", "<u2"), ("n_packets", "<u4"),
                         ("n_walked", "<u4"), ("n_resets", "<u4"), ("settled_after", "<u4"), ("settled_hit", "<u4"),
                         ("packets_observed", "<i4"), ("total_packets_observed", "<i4"), ("first_pkt_time", "<u4"),
                         ("first_offset", "<u8")])
assert SURVEY_DTYPE.itemsize == 64 and SURVEY_DTYPE.fields["first_offset"][1] == 56

# the follow stage (include/btbbx.h btbbx_follow_pkt / btbbx_follow_sum; follow.h checks the C layout with static_asserts)
FOLLOW_PKT_DTYPE = np.dtype([("piconet", "<u4"), ("clkn", "<u4"), ("stage", "u1"), ("channel", "u1"), ("hop_channel", "u1"),
                             ("on_hop", "u1"), ("job", "<u4")])
FOLLOW_SUM_DTYPE = np.dtype([("stage", "<u4"), ("job", "<u4"), ("n_hits", "<u4"), ("n_header", "<u4"), ("n_payload", "<u4"),
                             ("n_on_hop", "<u4"), ("n_off_hop", "<u4"), ("lt_addr_mask", "<u4")])
assert FOLLOW_PKT_DTYPE.itemsize == 16 and FOLLOW_SUM_DTYPE.itemsize == 32

_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32

# every symbol include/btbbx.h and include/btbb.h declare: (restype, argtypes)
SIGNATURES = {
    # ---- btbbx.h
    "btbbx_init": (C.c_int, [C.c_int]),
    "btbbx_init_devices": (C.c_int, [_vp, C.c_int, C.c_int]),
    "btbbx_shutdown": (None, []),
    "btbbx_last_error": (C.c_char_p, []),
    "btbbx_device_count": (C.c_int, []),
    "btbbx_table_errors": (C.c_int, []),
    "btbbx_slide_set": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "btbbx_slide_sets_two_level": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "btbbx_malloc": (_vp, [C.c_size_t]),
    "btbbx_free": (None, [_vp]),
    "btbbx_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_size_t]),
    "btbbx_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_size_t]),
    "btbbx_memset": (C.c_int, [_vp, C.c_int, C.c_size_t]),
    "btbbx_sync": (C.c_int, [_vp]),
    "btbbx_scan_device": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _u32, C.c_int, _vp, _u32, _vp, _vp]),
    "btbbx_scan_device_fmt": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _u32, C.c_int, C.c_int, _vp, _u32, _vp, _vp]),
    "btbbx_scan_first_device": (C.c_int, [_vp, _u64, _u64, _u32, C.c_int, _vp, _vp]),
    "btbbx_scan_host": (C.c_int64, [_vp, _u64, _u64, _u32, C.c_int, _vp, _u64]),
    "btbbx_scan_symbols": (C.c_int64, [_vp, _u64, _u64, _u32, C.c_int, _vp, _u64]),
    "btbbx_find_first_symbols": (C.c_int, [_vp, _u64, _u64, _u32, C.c_int, _vp]),
    "btbbx_shard_plan": (C.c_int, [_u64, _u32, _u32, _vp]),
    "btbbx_scan_host_multi": (C.c_int64, [_vp, _u64, _u64, _u32, C.c_int, _vp, _u64, _vp, C.c_int]),
    "btbbx_sort_hits": (None, [_vp, C.c_size_t]),
    "btbbx_sort_hits_device": (C.c_int, [_vp, _u32, _vp]),
    "btbbx_order_hits_scratch_bytes": (C.c_size_t, [_u32]),
    "btbbx_scan_ordered_scratch_bytes": (C.c_size_t, [_u64, _u32, _u32, _u32]),
    "btbbx_order_hits_device": (C.c_int, [_vp, _vp, _u32, _vp, C.c_size_t, _vp]),
    "btbbx_order_scan_hits_device": (C.c_int, [_vp, _vp, _u32, _u32, _u64, _vp, C.c_size_t, _vp]),
    "btbbx_scan_ordered_device": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _u32, C.c_int, _vp, _u32, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_scan_ordered_device_fmt": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _u32, C.c_int, C.c_int, _vp, _u32, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_pack_device": (C.c_int, [_vp, _u64, _vp, _vp]),
    "btbbx_unpack_device": (C.c_int, [_vp, _u64, _vp, _vp]),
    "btbbx_msb_to_lsb_device": (C.c_int, [_vp, _u64, _vp]),
    "btbbx_stream_open": (_vp, [_u32, C.c_int, _u64, C.c_int]),
    "btbbx_stream_feed": (C.c_int64, [_vp, _vp, _u64, _vp, _u64]),
    "btbbx_stream_acquire": (_vp, [_vp]),
    "btbbx_stream_submit": (C.c_int64, [_vp, _u64, _vp, _u64]),
    "btbbx_stream_flush": (C.c_int64, [_vp, _vp, _u64]),
    "btbbx_stream_close": (None, [_vp]),
    "btbbx_synth_device": (C.c_int, [_vp, _u64, _u64, _u64, _u32, C.c_int64, _u32, _vp]),
    "btbbx_gather_packets_device": (C.c_int, [_vp, _u64, _u64, _vp, _u32, _u32, _vp, _vp, _vp]),
    "btbbx_trials_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "btbbx_decode_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "btbbx_decode_hits_device": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "btbbx_decode_hits_counted_device": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "btbbx_decode_hits_piconet_device": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp]),
    "btbbx_decode_hits_piconet_phase_device": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "btbbx_uap_table_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "btbbx_hop_cfg_init": (None, [_vp, _u32, _vp]),
    "btbbx_hop_sequence_device": (C.c_int, [_vp, _u64, _u64, _vp, _vp]),
    "btbbx_hop_channels_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "btbbx_hop_reversal_open": (_vp, [_vp, _u32, C.c_uint8, C.c_int, C.POINTER(C.c_int)]),
    "btbbx_hop_reversal_winnow": (C.c_int, [_vp, _vp, _vp, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "btbbx_hop_reversal_candidates": (C.c_int64, [_vp, _vp, _u64]),
    "btbbx_hop_reversal_close": (None, [_vp]),
    "btbbx_hop_reversal_batch_scratch_bytes": (C.c_size_t, [_u32, _u32]),
    "btbbx_hop_reversal_batch_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, C.c_size_t, _vp]),
    "btbbx_hop_reversal_batch_host": (C.c_int64, [_vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32]),
    "btbbx_piconet_state": (C.c_int64, [_vp, C.c_int]),
    "btbbx_piconet_candidates": (C.c_int64, [_vp, _vp, _u64]),
    "btbbx_le_scan_device": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _u32, C.c_int, _vp, _u32, _vp, _vp]),
    "btbbx_le_decode_hits_device": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _u32, _vp, _u32, _vp, _vp]),
    "btbbx_le_scan_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, C.c_int, _vp, _u64]),
    "btbbx_le_coded_scan_device": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _u32, C.c_int, _vp, _u32, _vp, _vp]),
    "btbbx_le_coded_scratch_bytes": (C.c_size_t, [_u32]),
    "btbbx_le_coded_decode_hits_device": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_coded_scan_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, C.c_int, _vp, _vp, _u64]),
    "btbbx_le_cfind_scratch_bytes": (C.c_size_t, [_u32]),
    "btbbx_le_cfind_scan_device": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, C.c_int, _vp, _vp, _u32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_cfind_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, C.c_int, _u32, _vp, _u64, _vp, _u64, _vp]),
    "btbbx_le_ctrack_symbols_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _vp]),
    "btbbx_le_ctrack_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_ctrack_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, C.c_int, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                         _vp, _vp, _vp, _vp, _vp]),
    "btbbx_le_discover_scan_device": (C.c_int, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _vp, _u32, _vp, _vp]),
    "btbbx_le_discover_scratch_bytes": (C.c_size_t, [_u32]),
    "btbbx_le_discover_group_device": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_discover_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp]),
    "btbbx_le_track_scratch_bytes": (C.c_size_t, [_u32, _u32]),
    "btbbx_le_track_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_track_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                        _vp, _vp]),
    "btbbx_le_csa2_scratch_bytes": (C.c_size_t, [_u32, _u32]),
    "btbbx_le_csa2_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_csa2_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                       _vp, _vp, _vp, _vp]),
    "btbbx_le_seed_device": (C.c_int, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _vp]),
    "btbbx_le_epoch_scratch_bytes": (C.c_size_t, [_u32, _u32]),
    "btbbx_le_epoch_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _u32, _vp, _vp,
                                         _vp, C.c_size_t, _vp]),
    "btbbx_le_epoch_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                         C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "btbbx_le_span_scratch_bytes": (C.c_size_t, [_u32, _u32, _u32]),
    "btbbx_le_span_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _u32, _u32, _vp,
                                       _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_span_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                       C.c_int, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "btbbx_le_data_scratch_bytes": (C.c_size_t, [_u32, _u32]),
    "btbbx_le_data_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp,
                                       _vp, _u64, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_data_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                       _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "btbbx_le_crypt_scratch_bytes": (C.c_size_t, [_u32, _u32, _u32]),
    "btbbx_le_crypt_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp,
                                        _vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_crypt_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                        _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "btbbx_le_keyed_epoch_scratch_bytes": (C.c_size_t, [_u32, _u32]),
    "btbbx_le_keyed_epoch_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32,
                                               _u32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_keyed_span_scratch_bytes": (C.c_size_t, [_u32, _u32, _u32]),
    "btbbx_le_keyed_span_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32,
                                              _u32, _u32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_keyed_span_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                             C.c_int, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    "btbbx_le_pair_scratch_bytes": (C.c_size_t, [_u32]),
    "btbbx_le_pair_device": (C.c_int, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _u64, _u32, _vp, _vp, _u32, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_pair_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                       C.c_int, _vp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _u32, _vp]),
    "btbbx_le_resolve_scratch_bytes": (C.c_size_t, [_u32, _u32, _u32]),
    "btbbx_le_resolve_device": (C.c_int, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32,
                                          _vp, _vp, _vp, C.c_size_t, _vp]),
    "btbbx_le_resolve_adv_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, C.c_int, _vp, _u32, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _u32,
                                              _vp]),
    "btbbx_le_resolve_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _u32,
                                          C.c_int, _vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "btbbx_survey_scratch_bytes": (C.c_size_t, [_u32]),
    "btbbx_survey_hits_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp,
                                           _vp, C.c_size_t, _vp]),
    "btbbx_survey_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, C.c_int, _vp, _u32, _u32, _u32, _vp, _u64, _vp]),
    "btbbx_survey_clock_jobs_device": (C.c_int, [_vp, _vp, _u32, _vp, C.c_size_t, _u32, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp,
                                                 _vp, _vp, _vp, _u32, _vp, _vp]),
    "btbbx_acquire_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, C.c_int, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _u32, _u32,
                                       _vp, _vp, _vp, _u64, _vp, _vp, _u32]),
    "btbbx_follow_hits_device": (C.c_int, [_vp, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32,
                                           _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btbbx_follow_host": (C.c_int64, [_vp, _u64, _u64, _u32, _u64, C.c_int, _vp, _u32, _u32, _u32, _vp, _u64, _u32, _u32,
                                      _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    # ---- btbb.h
    "btbb_init": (C.c_int, [C.c_int]),
    "btbb_get_release": (C.c_char_p, []),
    "btbb_get_version": (C.c_char_p, []),
    "btbb_packet_new": (_vp, []),
    "btbb_packet_ref": (None, [_vp]),
    "btbb_packet_unref": (None, [_vp]),
    "btbb_find_ac": (C.c_int, [_vp, C.c_int, _u32, C.c_int, C.POINTER(_vp)]),
    "btbb_packet_set_flag": (None, [_vp, C.c_int, C.c_int]),
    "btbb_packet_get_flag": (C.c_int, [_vp, C.c_int]),
    "btbb_packet_get_lap": (_u32, [_vp]),
    "btbb_packet_set_uap": (None, [_vp, C.c_uint8]),
    "btbb_packet_get_uap": (C.c_uint8, [_vp]),
    "btbb_packet_get_nap": (C.c_uint16, [_vp]),
    "btbb_packet_set_modulation": (None, [_vp, C.c_uint8]),
    "btbb_packet_set_transport": (None, [_vp, C.c_uint8]),
    "btbb_packet_get_modulation": (C.c_uint8, [_vp]),
    "btbb_packet_get_transport": (C.c_uint8, [_vp]),
    "btbb_packet_get_channel": (C.c_uint8, [_vp]),
    "btbb_packet_get_ac_errors": (C.c_uint8, [_vp]),
    "btbb_packet_get_clkn": (_u32, [_vp]),
    "btbb_packet_get_header_packed": (_u32, [_vp]),
    "btbb_packet_set_data": (None, [_vp, _vp, C.c_int, C.c_uint8, _u32]),
    "btbb_get_symbols": (_vp, [_vp]),
    "btbb_packet_get_payload_length": (C.c_int, [_vp]),
    "btbb_get_payload": (_vp, [_vp]),
    "btbb_get_payload_packed": (C.c_int, [_vp, _vp]),
    "btbb_packet_get_type": (C.c_uint8, [_vp]),
    "btbb_packet_get_lt_addr": (C.c_uint8, [_vp]),
    "btbb_packet_get_header_flags": (C.c_uint8, [_vp]),
    "btbb_packet_get_hec": (C.c_uint8, [_vp]),
    "btbb_gen_syncword": (_u64, [C.c_int]),
    "btbb_decode_header": (C.c_int, [_vp]),
    "btbb_decode_payload": (C.c_int, [_vp]),
    "btbb_print_packet": (None, [_vp]),
    "btbb_header_present": (C.c_int, [_vp]),
    "try_clock": (C.c_uint8, [C.c_int, _vp]),
    "crc_check": (C.c_int, [C.c_int, _vp]),
    "lap_from_fhs": (_u32, [_vp]),
    "uap_from_fhs": (C.c_uint8, [_vp]),
    "nap_from_fhs": (C.c_uint16, [_vp]),
    "clock_from_fhs": (_u32, [_vp]),
    "tun_format": (_vp, [_vp]),
    "btbb_piconet_new": (_vp, []),
    "btbb_piconet_ref": (None, [_vp]),
    "btbb_piconet_unref": (None, [_vp]),
    "btbb_init_piconet": (None, [_vp, _u32]),
    "btbb_piconet_set_uap": (None, [_vp, C.c_uint8]),
    "btbb_piconet_get_uap": (C.c_uint8, [_vp]),
    "btbb_piconet_get_lap": (_u32, [_vp]),
    "btbb_piconet_get_nap": (C.c_uint16, [_vp]),
    "btbb_piconet_get_bdaddr": (_u64, [_vp]),
    "btbb_piconet_get_clk_offset": (C.c_int, [_vp]),
    "btbb_piconet_set_clk_offset": (None, [_vp, C.c_int]),
    "btbb_piconet_set_flag": (None, [_vp, C.c_int, C.c_int]),
    "btbb_piconet_get_flag": (C.c_int, [_vp, C.c_int]),
    "btbb_piconet_set_channel_seen": (C.c_uint8, [_vp, C.c_uint8]),
    "btbb_piconet_clear_channel_seen": (C.c_uint8, [_vp, C.c_uint8]),
    "btbb_piconet_get_channel_seen": (C.c_uint8, [_vp, C.c_uint8]),
    "btbb_piconet_get_afh_map": (_vp, [_vp]),
    "btbb_process_packet": (C.c_int, [_vp, _vp]),
    "btbb_uap_from_header": (C.c_int, [_vp, _vp]),
    "btbb_print_afh_map": (None, [_vp]),
    "btbb_piconet_set_afh_map": (None, [_vp, _vp]),
    "btbb_init_hop_reversal": (C.c_int, [C.c_int, _vp]),
    "btbb_winnow": (C.c_int, [_vp]),
    "btbb_pcapng_create_file": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(_vp)]),
    "btbb_pcapng_append_packet": (C.c_int, [_vp, _u64, C.c_int8, C.c_int8, _u32, C.c_uint8, _vp]),
    "btbb_pcapng_record_bdaddr": (C.c_int, [_vp, _u64, C.c_uint8, C.c_uint8]),
    "btbb_pcapng_record_btclock": (C.c_int, [_vp, _u64, _u64, _u32, _u32]),
    "btbb_pcapng_close": (C.c_int, [_vp]),
    "btbb_pcap_create_file": (C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    "btbb_pcap_append_packet": (C.c_int, [_vp, _u64, C.c_int8, C.c_int8, _u32, C.c_uint8, _vp]),
    "btbb_pcap_close": (C.c_int, [_vp]),
    "btbb_decode": (C.c_int, [_vp]),
    "btbb_init_survey": (C.c_int, []),
    "btbb_next_survey_result": (_vp, []),
}

_lib = None


class BtbbError(RuntimeError):
    pass


def lib():
    """The loaded C-ABI library (raises if it has not been built -- no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BtbbError(
                "%s is missing: build it with `make -C libbtbb_amd/csrc` "
                "(or __graft_entry__.build()); there is no Python/CPU fallback" % LIB_PATH)
        handle = C.CDLL(LIB_PATH)          # RTLD_LOCAL: same symbol names as the reference checker
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what="btbbx call"):
    if rc < 0:
        raise BtbbError("%s failed (%d): %s" % (what, rc, lib().btbbx_last_error().decode()))
    return rc


def init(max_ac_errors=2):
    """btbb_init() on the current HIP device."""
    check(lib().btbbx_init(max_ac_errors), "btbbx_init")


def _ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------
# thin host-buffer helpers (tests, small jobs); the benchmark uses the *_device entries
# ------------------------------------------------------------------------------------
def init_devices(devices, max_ac_errors=2):
    """btbb_init() on every listed HIP device (for scan_words_multi)."""
    arr = (C.c_int * len(devices))(*devices)
    check(lib().btbbx_init_devices(arr, len(devices), max_ac_errors), "btbbx_init_devices")


def shard_plan(search_bits, n_shards, shard):
    """The library's time-shard plan (btbbx_shard_plan): which words shard `shard` of `n_shards` reads."""
    out = Shard()
    check(lib().btbbx_shard_plan(search_bits, n_shards, shard, C.byref(out)), "btbbx_shard_plan")
    return dict(first_word=out.first_word, n_words=out.n_words, search_bits=out.search_bits,
                first_offset=out.first_offset)


def scan_words(words, search_bits, lap=LAP_ANY, max_ac_errors=2, cap=1 << 20, truncate=False):
    """All access codes in a packed stream held in host memory (numpy uint64).  With truncate=True
    the `cap` smallest (stream, offset) hits are returned when more were found."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    hits = np.zeros(cap, dtype=HIT_DTYPE)
    n = check(lib().btbbx_scan_host(_ptr(words), len(words), search_bits, lap, max_ac_errors, _ptr(hits), cap),
              "btbbx_scan_host")
    if n > cap and not truncate:
        raise BtbbError("hit buffer too small: %d > %d" % (n, cap))
    return hits[:min(n, cap)]


def scan_words_multi(words, search_bits, devices, lap=LAP_ANY, max_ac_errors=2, cap=1 << 20, truncate=False):
    """The same through btbbx_scan_host_multi: the capture is time-sharded over `devices` (HIP ordinals,
    repeats allowed), one host thread per entry."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    hits = np.zeros(cap, dtype=HIT_DTYPE)
    arr = (C.c_int * len(devices))(*devices)
    n = check(lib().btbbx_scan_host_multi(_ptr(words), len(words), search_bits, lap, max_ac_errors, _ptr(hits), cap,
                                          arr, len(devices)), "btbbx_scan_host_multi")
    if n > cap and not truncate:
        raise BtbbError("hit buffer too small: %d > %d" % (n, cap))
    return hits[:min(n, cap)]


def scan_symbols(symbols, search_length, lap=LAP_ANY, max_ac_errors=2, cap=1 << 20):
    symbols = np.ascontiguousarray(symbols, dtype=np.uint8)
    hits = np.zeros(cap, dtype=HIT_DTYPE)
    n = check(lib().btbbx_scan_symbols(_ptr(symbols), len(symbols), search_length, lap, max_ac_errors,
                                       _ptr(hits), cap), "btbbx_scan_symbols")
    if n > cap:
        raise BtbbError("hit buffer too small: %d > %d" % (n, cap))
    return hits[:n]


def le_scan(words, search_bits, phys_channels, aa=LE_ADV_AA, crc_init=LE_ADV_CRC_INIT, max_errors=2, n_streams=1,
            pitch_words=None, n_words=None, cap=1 << 20, truncate=False):
    """Bluetooth LE packets (preamble + access address within max_errors bit errors, dewhitened, CRC checked) in
    n_streams packed streams held in host memory: words is (n_streams, pitch_words) or flat, each stream's first n_words
    words (default: all pitch_words) are its bits; phys_channels = the RF MHz of every stream.  Returns LE_PKT_DTYPE records in (stream, offset) order.  With truncate=True the `cap` smallest
    (stream, offset) records are returned when more were found."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    pkts = np.zeros(max(cap, 1), dtype=LE_PKT_DTYPE)
    n = check(lib().btbbx_le_scan_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), aa, crc_init,
                                       max_errors, _ptr(pkts), cap), "btbbx_le_scan_host")
    if n > cap and not truncate:
        raise BtbbError("packet buffer too small: %d > %d" % (n, cap))
    return pkts[:min(n, cap)]


def le_coded_scan(words, search_bits, phys_channels, aa=LE_ADV_AA, crc_init=LE_ADV_CRC_INIT, max_errors=16, n_streams=1,
                  pitch_words=None, n_words=None, cap=1 << 20, truncate=False):
    """Bluetooth LE Coded PHY packets (include/btbbx.h, LE Coded PHY scan: the 336 symbols preamble + coded access address within
    max_errors <= 63 mismatches, both FEC blocks Viterbi-decoded, dewhitened, CRC checked) in n_streams packed streams held in host
    memory; words, phys_channels, n_words and pitch_words as le_scan.  Returns (pkts, info): LE_PKT_DTYPE and LE_CODED_INFO_DTYPE
    records of the same hits in (stream, offset) order.  With truncate=True the `cap` smallest are returned when more were found."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    pkts = np.zeros(max(cap, 1), dtype=LE_PKT_DTYPE)
    info = np.zeros(max(cap, 1), dtype=LE_CODED_INFO_DTYPE)
    n = check(lib().btbbx_le_coded_scan_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), aa, crc_init,
                                             max_errors, _ptr(pkts), _ptr(info), cap), "btbbx_le_coded_scan_host")
    if n > cap and not truncate:
        raise BtbbError("packet buffer too small: %d > %d" % (n, cap))
    return pkts[:min(n, cap)], info[:min(n, cap)]


def le_discover(words, search_bits, phys_channels, max_len=27, min_count=2, n_streams=1, pitch_words=None, n_words=None,
                conn_cap=1 << 16, cand_cap=1 << 20, truncate=False):
    """The Bluetooth LE connections of a data-channel capture, neither access address nor CRCInit given: every candidate
    packet (include/btbbx.h: preamble rule, an access address without offense, a plausible header of length <= max_len, the
    CRCInit that makes its CRC come out) grouped by (access address, CRCInit).  words / n_streams / pitch_words / n_words /
    phys_channels as le_scan.  Returns (conns, cands): LE_CONN_DTYPE records of the groups with at least min_count members in
    ascending (AA, CRCInit) order, and the LE_CAND_DTYPE candidates sorted by (AA, CRCInit, stream, offset), each with the index
    of its connection in `conn` (LE_NO_CONN: none).  With truncate=True the first conn_cap / cand_cap records are returned when
    more were found."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)          # (not zeroed: only the records returned are ever touched)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_discover_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                           _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands)), "btbbx_le_discover_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    return conns[:min(n, conn_cap)].copy(), cands[:min(n_cands.value, cand_cap)].copy()


def le_coded_discover(words, search_bits, phys_channels, max_len=27, max_errors=16, min_count=2, n_streams=1, pitch_words=None,
                      n_words=None, conn_cap=1 << 16, cand_cap=1 << 20, truncate=False):
    """The LE Coded PHY connections of a data-channel capture, neither access address nor CRCInit given (include/btbbx.h,
    promiscuous LE Coded connection discovery, rules 1..12): every offset whose block 1 decodes to an access address without
    offense that the 336 symbols match within max_errors <= 63, with a plausible header of length <= max_len, a packet that fits and
    the CRCInit that makes its CRC come out, grouped by (access address, CRCInit) by le_discover's grouping.  Arguments and the
    returned (conns, cands) -- LE_CONN_DTYPE and LE_CAND_DTYPE -- as le_discover."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)          # (not zeroed: only the records returned are ever touched)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_cfind_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, max_errors,
                                        min_count, _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands)), "btbbx_le_cfind_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    return conns[:min(n, conn_cap)].copy(), cands[:min(n_cands.value, cand_cap)].copy()


def le_track(words, search_bits, phys_channels, max_len=27, min_count=2, n_streams=1, pitch_words=None, n_words=None,
             unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, conn_cap=1 << 12, cand_cap=1 << 20, truncate=False):
    """le_discover, then the tracking of every connection it stored (include/btbbx.h btbbx_le_track_device): events, connection
    interval, event counters, hop increment and the hop check of every packet.  unit_bits: the bits of 1.25 ms; ifs_bits: the
    longest gap between the packets of one connection event; jitter_bits: how far an event spacing may lie from the 1.25 ms
    grid.  Returns (conns, cands, tracks, pkts): le_discover's two arrays, LE_TRACK_DTYPE records parallel to conns and
    LE_TRACK_PKT_DTYPE records parallel to cands."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_track_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                        _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                        flags, _ptr(tracks), _ptr(pkts)), "btbbx_le_track_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy()


def le_csa2(words, search_bits, phys_channels, max_len=27, min_count=2, n_streams=1, pitch_words=None, n_words=None,
            unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_CSA2_REMAP, conn_cap=1 << 12, cand_cap=1 << 20, truncate=False):
    """le_track, then channel selection algorithm #2 for every connection it timed (include/btbbx.h btbbx_le_csa2_device): the
    absolute connEventCounter of the first event seen, the channel predicted for every packet, and whether #2 explains the
    connection better than #1.  le_track's parameters; bit 0 of flags serves both stages.  Returns (conns, cands, tracks, pkts, sel,
    sel_pkts): le_track's four arrays, LE_CSA2_DTYPE records parallel to conns and LE_CSA2_PKT_DTYPE records parallel to cands."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    sel = np.empty(max(conn_cap, 1), dtype=LE_CSA2_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    sel_pkts = np.empty(max(cand_cap, 1), dtype=LE_CSA2_PKT_DTYPE)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_csa2_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                       _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                       flags, _ptr(tracks), _ptr(pkts), _ptr(sel), _ptr(sel_pkts)), "btbbx_le_csa2_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), sel[:nc].copy(), sel_pkts[:nk].copy()


def le_coded_track(words, search_bits, phys_channels, max_len=27, max_errors=16, min_count=2, n_streams=1, pitch_words=None, n_words=None,
                   unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_CSA2_REMAP, conn_cap=1 << 12, cand_cap=1 << 20, truncate=False):
    """le_coded_discover, then the duration of every coded candidate, the tracking with rule 3 taking it and channel selection
    algorithm #2 (include/btbbx.h, LE Coded connection tracking: btbbx_le_ctrack_host).  le_coded_discover's and le_csa2's parameters.
    Returns what le_csa2 returns, plus symbols: (conns, cands, tracks, pkts, sel, sel_pkts, symbols), symbols a uint32 array
    parallel to cands -- 376 + S * (8 * (length + 5) + 3) symbols from the first preamble symbol."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    sel = np.empty(max(conn_cap, 1), dtype=LE_CSA2_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    sel_pkts = np.empty(max(cand_cap, 1), dtype=LE_CSA2_PKT_DTYPE)
    symbols = np.empty(max(cand_cap, 1), dtype=np.uint32)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_ctrack_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, max_errors, min_count,
                                         _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                         flags, _ptr(tracks), _ptr(pkts), _ptr(sel), _ptr(sel_pkts), _ptr(symbols)), "btbbx_le_ctrack_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), sel[:nc].copy(), sel_pkts[:nk].copy(), symbols[:nk].copy()


def le_follow(words, search_bits, phys_channels, max_len=27, min_count=2, n_streams=1, pitch_words=None, n_words=None,
              unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, adv_errors=0, conn_cap=1 << 12, cand_cap=1 << 20,
              truncate=False):
    """le_track, then LE following from CONNECT_IND (include/btbbx.h btbbx_le_seed_device / btbbx_le_epoch_device): every
    connection joined with the CONNECT_IND on an advertising stream of the same capture (adv_errors: mismatches allowed over its
    preamble and access address), every event's absolute connEventCounter, the channel map updates put in force at their instants,
    and every packet checked against the prediction of the map in force.  le_track's parameters.  Returns (conns, cands, tracks,
    pkts, seeds, follows, follow_pkts): le_track's four arrays, LE_SEED_DTYPE and LE_FOLLOW_DTYPE records parallel to conns and
    LE_FOLLOW_PKT_DTYPE records parallel to cands."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    seeds = np.empty(max(conn_cap, 1), dtype=LE_SEED_DTYPE)
    follows = np.empty(max(conn_cap, 1), dtype=LE_FOLLOW_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    follow_pkts = np.empty(max(cand_cap, 1), dtype=LE_FOLLOW_PKT_DTYPE)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_epoch_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                         _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                         flags, adv_errors, _ptr(tracks), _ptr(pkts), _ptr(seeds), _ptr(follows), _ptr(follow_pkts)),
              "btbbx_le_epoch_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return (conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), seeds[:nc].copy(), follows[:nc].copy(),
            follow_pkts[:nk].copy())


def le_span(words, search_bits, phys_channels, max_len=27, min_count=2, n_streams=1, pitch_words=None, n_words=None,
            unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, adv_errors=0, conn_cap=1 << 12, cand_cap=1 << 20,
            truncate=False, max_updates=4):
    """le_follow's chain with the span stage in the follow stage's place (include/btbbx.h btbbx_le_span_device): counters, map
    updates and the hop check carried through up to max_updates (0..16) connection parameter updates per connection.  le_follow's
    parameters.  Returns (conns, cands, tracks, pkts, seeds, spans, span_pkts, span_recs): le_follow's arrays up to seeds,
    LE_SPAN_DTYPE records parallel to conns, LE_SPAN_PKT_DTYPE records parallel to cands and LE_SPAN_REC_DTYPE records of shape
    (connections, max_updates + 1)."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    per = min(int(max_updates), 16) + 1
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    seeds = np.empty(max(conn_cap, 1), dtype=LE_SEED_DTYPE)
    spans = np.empty(max(conn_cap, 1), dtype=LE_SPAN_DTYPE)
    span_recs = np.empty((max(conn_cap, 1), per), dtype=LE_SPAN_REC_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    span_pkts = np.empty(max(cand_cap, 1), dtype=LE_SPAN_PKT_DTYPE)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_span_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                       _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                       flags, adv_errors, _ptr(tracks), _ptr(pkts), _ptr(seeds), max_updates, _ptr(spans), _ptr(span_pkts),
                                       _ptr(span_recs)), "btbbx_le_span_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return (conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), seeds[:nc].copy(), spans[:nc].copy(),
            span_pkts[:nk].copy(), span_recs[:nc].copy())


def le_data(words, search_bits, phys_channels, max_len=27, min_count=2, n_streams=1, pitch_words=None, n_words=None,
            unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, conn_cap=1 << 12, cand_cap=1 << 20, truncate=False,
            msg_cap=1 << 16, byte_cap=1 << 22):
    """le_track, then the data of every connection it stored (include/btbbx.h btbbx_le_data_device): every packet's role, SN / NESN /
    MD bits and whether it is new or a retransmission, and the L2CAP messages of either direction reassembled from their fragments.
    le_track's parameters; msg_cap and byte_cap: the message records and payload octets to keep (without truncate, more of either
    raises).  Returns (conns, cands, tracks, pkts, data, data_pkts, msgs, payload): le_track's four arrays, LE_DATA_DTYPE records
    parallel to conns, LE_DATA_PKT_DTYPE records parallel to cands, the LE_MSG_DTYPE records and the uint8 buffer their byte_offset
    points into, cut to the stored messages."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    data = np.empty(max(conn_cap, 1), dtype=LE_DATA_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    data_pkts = np.empty(max(cand_cap, 1), dtype=LE_DATA_PKT_DTYPE)
    msgs = np.empty(max(msg_cap, 1), dtype=LE_MSG_DTYPE)
    payload = np.empty(max(byte_cap, 1), dtype=np.uint8)
    n_cands, n_msgs, n_bytes = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    n = check(lib().btbbx_le_data_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                       _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                       flags, _ptr(tracks), _ptr(pkts), _ptr(data), _ptr(data_pkts), _ptr(msgs), msg_cap, C.byref(n_msgs),
                                       _ptr(payload), byte_cap, C.byref(n_bytes)), "btbbx_le_data_host")
    if (n > conn_cap or n_cands.value > cand_cap or n_msgs.value > msg_cap or n_bytes.value > byte_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d, %d candidates > %d, %d messages > %d or %d octets > %d" % (
            n, conn_cap, n_cands.value, cand_cap, n_msgs.value, msg_cap, n_bytes.value, byte_cap))
    nc, nk, nm = min(n, conn_cap), min(n_cands.value, cand_cap), min(n_msgs.value, msg_cap)
    msgs = msgs[:nm].copy()
    stored = msgs[(msgs["flags"] & LE_MSG_STORED) != 0]
    kept = int(stored["byte_offset"][-1]) + int(stored["bytes"][-1]) if len(stored) else 0
    return (conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), data[:nc].copy(), data_pkts[:nk].copy(), msgs,
            payload[:kept].copy())


def le_decrypt(words, search_bits, phys_channels, keys, window=8, max_len=27, min_count=2, n_streams=1, pitch_words=None, n_words=None,
               unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, conn_cap=1 << 12, cand_cap=1 << 20, truncate=False,
               msg_cap=1 << 16, byte_cap=1 << 22):
    """le_data, then the decryption of every connection whose encryption start is in the capture (include/btbbx.h
    btbbx_le_crypt_device).  keys: the candidate long-term keys, 1 to 64 of them, each 16 octets most significant octet first, as
    bytes objects or one (n, 16) uint8 array; window: the packet counter skews 0 .. window - 1 that are tried per packet (1..32).
    An encrypted PDU is 4 octets longer than its plaintext and max_len is NOT raised for the caller: the discovery's default of 27
    drops every encrypted PDU of more than 23 plaintext octets.  Pass max_len >= 31 for a connection of 27-octet PDUs and 255 with
    data length extension.
    Returns (conns, cands, tracks, pkts, data, data_pkts, msgs, payload, crypt, crypt_pkts, plain_pkts): le_data's tuple, in which
    data and data_pkts are the data stage's records and msgs and payload the messages over PLAINTEXT (rule 8), then LE_CRYPT_DTYPE
    records parallel to conns, LE_CRYPT_PKT_DTYPE records parallel to cands and the LE_DATA_PKT_DTYPE records under the effective
    members, parallel to cands."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    if not isinstance(keys, np.ndarray):
        keys = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8)
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    data = np.empty(max(conn_cap, 1), dtype=LE_DATA_DTYPE)
    crypt = np.empty(max(conn_cap, 1), dtype=LE_CRYPT_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    data_pkts = np.empty(max(cand_cap, 1), dtype=LE_DATA_PKT_DTYPE)
    crypt_pkts = np.empty(max(cand_cap, 1), dtype=LE_CRYPT_PKT_DTYPE)
    plain_pkts = np.empty(max(cand_cap, 1), dtype=LE_DATA_PKT_DTYPE)
    msgs = np.empty(max(msg_cap, 1), dtype=LE_MSG_DTYPE)
    payload = np.empty(max(byte_cap, 1), dtype=np.uint8)
    n_cands, n_msgs, n_bytes = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    n = check(lib().btbbx_le_crypt_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                        _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                        flags, _ptr(tracks), _ptr(pkts), _ptr(data), _ptr(data_pkts), _ptr(keys), len(keys), window,
                                        _ptr(crypt), _ptr(crypt_pkts), _ptr(plain_pkts), _ptr(msgs), msg_cap, C.byref(n_msgs),
                                        _ptr(payload), byte_cap, C.byref(n_bytes)), "btbbx_le_crypt_host")
    if (n > conn_cap or n_cands.value > cand_cap or n_msgs.value > msg_cap or n_bytes.value > byte_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d, %d candidates > %d, %d messages > %d or %d octets > %d" % (
            n, conn_cap, n_cands.value, cand_cap, n_msgs.value, msg_cap, n_bytes.value, byte_cap))
    nc, nk, nm = min(n, conn_cap), min(n_cands.value, cand_cap), min(n_msgs.value, msg_cap)
    msgs = msgs[:nm].copy()
    stored = msgs[(msgs["flags"] & LE_MSG_STORED) != 0]
    kept = int(stored["byte_offset"][-1]) + int(stored["bytes"][-1]) if len(stored) else 0
    return (conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), data[:nc].copy(), data_pkts[:nk].copy(), msgs,
            payload[:kept].copy(), crypt[:nc].copy(), crypt_pkts[:nk].copy(), plain_pkts[:nk].copy())


def le_pair(words, search_bits, phys_channels, tk_limit=LE_PAIR_MAX_TK, key_cap=LE_PAIR_MAX_KEYS, max_len=27, min_count=2, n_streams=1,
            pitch_words=None, n_words=None, unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, adv_errors=0,
            conn_cap=1 << 12, cand_cap=1 << 20, truncate=False, msg_cap=1 << 16, byte_cap=1 << 22):
    """le_follow's chain up to the seeds, then the data stage and LE legacy pairing key recovery (include/btbbx.h
    btbbx_le_pair_device): for every connection whose CONNECT_IND and Security Manager exchange are in the capture the temporary key
    -- every value below tk_limit (0..1000000; 1: Just Works only, 0: search nothing) is tried against the Confirm values -- and the
    short-term key under it.  key_cap (0..64): the slots of the key table; msg_cap and byte_cap: the device-side room for the
    messages that are searched for the exchange, which are not returned.  le_follow's other parameters.
    Returns (conns, cands, tracks, pkts, seeds, pairs, keys, n_keys): le_follow's arrays up to seeds, LE_PAIR_DTYPE records parallel
    to conns, the key table as a (key_cap, 16) uint8 array in the byte order le_decrypt takes, unused slots zero, and the number of
    connections with a short-term key, which may exceed key_cap."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    seeds = np.empty(max(conn_cap, 1), dtype=LE_SEED_DTYPE)
    pairs = np.empty(max(conn_cap, 1), dtype=LE_PAIR_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    keys = np.zeros((max(key_cap, 1), 16), dtype=np.uint8)
    n_cands, n_keys = C.c_uint64(0), C.c_uint32(0)
    n = check(lib().btbbx_le_pair_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                       _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                       flags, adv_errors, _ptr(tracks), _ptr(pkts), _ptr(seeds), msg_cap, byte_cap, tk_limit, _ptr(pairs),
                                       _ptr(keys), key_cap, C.byref(n_keys)), "btbbx_le_pair_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return (conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), seeds[:nc].copy(), pairs[:nc].copy(),
            keys[:key_cap].copy(), int(n_keys.value))


def le_crack(words, search_bits, phys_channels, tk_limit=LE_PAIR_MAX_TK, key_cap=LE_PAIR_MAX_KEYS, window=8, adv_errors=0, **kw):
    """le_pair, then le_decrypt under the short-term keys it recovered: capture in, plaintext out, no key given.  kw: what both take
    (max_len, min_count, n_streams, pitch_words, n_words, the timing, flags, the caps, truncate); max_len is le_decrypt's, see there.
    Returns (pair, plain): le_pair's tuple and le_decrypt's.  When no key was found nothing is raised and plain is None."""
    pair = le_pair(words, search_bits, phys_channels, tk_limit=tk_limit, key_cap=key_cap, adv_errors=adv_errors, **kw)
    found = min(pair[7], key_cap)
    if not found:
        return pair, None
    return pair, le_decrypt(words, search_bits, phys_channels, pair[6][:found], window=window, **kw)


def le_span_keyed(words, search_bits, phys_channels, keys, window=8, max_updates=4, max_len=27, min_count=2, n_streams=1,
                  pitch_words=None, n_words=None, unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, adv_errors=0,
                  conn_cap=1 << 12, cand_cap=1 << 20, truncate=False):
    """le_span's chain with the data stage, the decryption stage under `keys` and `window` (le_decrypt's) and the KEYED span stage
    behind the seeds (include/btbbx.h btbbx_le_keyed_span_device): the channel map and connection parameter updates a connection
    sends encrypted are read as plaintext and put in force.  le_span's other parameters.  max_len is not raised: an encrypted PDU is
    4 octets longer than its plaintext, so pass max_len >= 31 for a connection with 27-octet PDUs (an encrypted parameter update
    itself is 16 octets long) and 255 with data length extension.
    Returns (conns, cands, tracks, pkts, seeds, crypt, crypt_pkts, spans, span_pkts, span_recs): le_span's arrays with the
    LE_CRYPT_DTYPE records parallel to conns and the LE_CRYPT_PKT_DTYPE records parallel to cands behind the seeds."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    if not isinstance(keys, np.ndarray):
        keys = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8)
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)
    per = min(int(max_updates), 16) + 1
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    seeds = np.empty(max(conn_cap, 1), dtype=LE_SEED_DTYPE)
    crypt = np.empty(max(conn_cap, 1), dtype=LE_CRYPT_DTYPE)
    spans = np.empty(max(conn_cap, 1), dtype=LE_SPAN_DTYPE)
    span_recs = np.empty((max(conn_cap, 1), per), dtype=LE_SPAN_REC_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    crypt_pkts = np.empty(max(cand_cap, 1), dtype=LE_CRYPT_PKT_DTYPE)
    span_pkts = np.empty(max(cand_cap, 1), dtype=LE_SPAN_PKT_DTYPE)
    n_cands = C.c_uint64(0)
    n = check(lib().btbbx_le_keyed_span_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                             _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits,
                                             jitter_bits, flags, adv_errors, _ptr(tracks), _ptr(pkts), _ptr(seeds), _ptr(keys), len(keys),
                                             window, _ptr(crypt), _ptr(crypt_pkts), max_updates, _ptr(spans), _ptr(span_pkts),
                                             _ptr(span_recs)), "btbbx_le_keyed_span_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return (conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), seeds[:nc].copy(), crypt[:nc].copy(),
            crypt_pkts[:nk].copy(), spans[:nc].copy(), span_pkts[:nk].copy(), span_recs[:nc].copy())


def le_crack_span(words, search_bits, phys_channels, tk_limit=LE_PAIR_MAX_TK, key_cap=LE_PAIR_MAX_KEYS, window=8, max_updates=4,
                  adv_errors=0, **kw):
    """le_pair, then le_span_keyed under the short-term keys it recovered, as le_crack composes pairing and decryption: capture in,
    every connection followed through the updates it sends encrypted, no key given.  kw: what both take (max_len, min_count,
    n_streams, pitch_words, n_words, the timing, flags, conn_cap, cand_cap, truncate); msg_cap and byte_cap go to le_pair alone.
    Returns (pair, keyed): le_pair's tuple and le_span_keyed's.  When no key was found nothing is raised and keyed is None."""
    pair = le_pair(words, search_bits, phys_channels, tk_limit=tk_limit, key_cap=key_cap, adv_errors=adv_errors, **kw)
    found = min(pair[7], key_cap)
    if not found:
        return pair, None
    kw = {k: v for k, v in kw.items() if k not in ("msg_cap", "byte_cap")}
    return pair, le_span_keyed(words, search_bits, phys_channels, pair[6][:found], window=window, max_updates=max_updates,
                               adv_errors=adv_errors, **kw)


def _key_rows(keys):
    """Keys as a (n, 16) uint8 array: an array, or a sequence of 16-octet values."""
    if keys is None:
        return np.zeros((0, 16), np.uint8)
    if not isinstance(keys, np.ndarray):
        keys = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8)
    return np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)


def le_resolve(words, search_bits, phys_channels, irks, adv_errors=0, n_streams=1, pitch_words=None, n_words=None, adv_cap=1 << 20,
               addr_cap=1 << 20, irk_cap=None, truncate=False):
    """LE address resolution over the advertising channels alone (include/btbbx.h btbbx_le_resolve_device): the advertising scan
    (le_scan's, with adv_errors), then every distinct device address of the advertising PDUs and every resolvable private address
    among them tried against `irks` (16-octet keys in AES key order, most significant octet first, at most 4096).  irk_cap: the
    table's slots, len(irks) by default.  The capture needs no data channel.
    Returns (adv, slot_addr, addrs, table): the LE_PKT_DTYPE records in (stream, offset) order, a (len(adv), 2) uint32 array with the rank of each
    record's two address slots in addrs (LE_NO_ADDR: the slot holds none), the LE_ADDR_DTYPE records ascending by (random bit,
    address) -- irk names the smallest matching slot of the table, LE_NO_IRK if none -- and the LE_IRK_DTYPE records of the table."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    given = _key_rows(irks)
    irk_cap = len(given) if irk_cap is None else irk_cap
    adv = np.empty(max(adv_cap, 1), dtype=LE_PKT_DTYPE)
    slot_addr = np.empty((max(adv_cap, 1), 2), dtype=np.uint32)
    addrs = np.empty(max(addr_cap, 1), dtype=LE_ADDR_DTYPE)
    table = np.empty(max(irk_cap, 1), dtype=LE_IRK_DTYPE)
    n_addrs, n_irks = C.c_uint32(0), C.c_uint32(0)
    n = check(lib().btbbx_le_resolve_adv_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), adv_errors, _ptr(given),
                                              len(given), _ptr(adv), adv_cap, _ptr(slot_addr), _ptr(addrs), addr_cap, C.byref(n_addrs),
                                              _ptr(table), irk_cap, C.byref(n_irks)), "btbbx_le_resolve_adv_host")
    if (n > adv_cap or n_addrs.value > addr_cap) and not truncate:
        raise BtbbError("buffers too small: %d advertising records > %d or %d addresses > %d" % (n, adv_cap, n_addrs.value, addr_cap))
    na = min(n, adv_cap)
    return adv[:na].copy(), slot_addr[:na].copy(), addrs[:min(n_addrs.value, addr_cap)].copy(), table[:irk_cap].copy()


def le_identify(words, search_bits, phys_channels, keys, irks=None, window=8, max_len=27, min_count=2, n_streams=1, pitch_words=None,
                n_words=None, unit_bits=1250, ifs_bits=200, jitter_bits=50, flags=LE_TRACK_REMAP, adv_errors=0, conn_cap=1 << 12,
                cand_cap=1 << 20, truncate=False, msg_cap=1 << 16, byte_cap=1 << 22, irk_cap=LE_RESOLVE_MAX_IRKS, addr_cap=1 << 16):
    """le_span_keyed's chain up to and including the decryption stage under `keys` and `window` (le_decrypt's), then LE address
    resolution (include/btbbx.h btbbx_le_resolve_device) over the decrypted messages, the chain's own advertising records and the
    caller's `irks` (may be None): the identity resolving keys the peers distribute are read out of the plaintext, and every
    resolvable private address of the advertising channels is tried against them and the caller's.  msg_cap and byte_cap: the
    device-side room for the decrypted messages, which are not returned.  le_follow's other parameters; max_len as le_span_keyed.
    Returns (conns, cands, tracks, pkts, seeds, peers, table, addrs, n_irks, n_addrs): le_follow's arrays up to seeds, LE_PEER_DTYPE
    records parallel to conns, the LE_IRK_DTYPE table (irk_cap records: the caller's keys, then the harvested ones), the first
    addr_cap LE_ADDR_DTYPE records and the two counts, which may exceed their caps."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    phys = np.ascontiguousarray(np.broadcast_to(np.asarray(phys_channels, dtype=np.uint16), (n_streams,)))
    keys, given = _key_rows(keys), _key_rows(irks)
    conns = np.empty(max(conn_cap, 1), dtype=LE_CONN_DTYPE)
    tracks = np.empty(max(conn_cap, 1), dtype=LE_TRACK_DTYPE)
    seeds = np.empty(max(conn_cap, 1), dtype=LE_SEED_DTYPE)
    peers = np.empty(max(conn_cap, 1), dtype=LE_PEER_DTYPE)
    cands = np.empty(max(cand_cap, 1), dtype=LE_CAND_DTYPE)
    pkts = np.empty(max(cand_cap, 1), dtype=LE_TRACK_PKT_DTYPE)
    table = np.zeros(max(irk_cap, 1), dtype=LE_IRK_DTYPE)
    addrs = np.zeros(max(addr_cap, 1), dtype=LE_ADDR_DTYPE)
    n_cands, n_irks, n_addrs = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    n = check(lib().btbbx_le_resolve_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, _ptr(phys), max_len, min_count,
                                          _ptr(conns), conn_cap, _ptr(cands), cand_cap, C.byref(n_cands), unit_bits, ifs_bits, jitter_bits,
                                          flags, adv_errors, _ptr(tracks), _ptr(pkts), _ptr(seeds), _ptr(keys), len(keys), window, msg_cap,
                                          byte_cap, _ptr(given), len(given), _ptr(peers), _ptr(table), irk_cap, C.byref(n_irks), _ptr(addrs),
                                          addr_cap, C.byref(n_addrs)), "btbbx_le_resolve_host")
    if (n > conn_cap or n_cands.value > cand_cap) and not truncate:
        raise BtbbError("buffers too small: %d connections > %d or %d candidates > %d" % (n, conn_cap, n_cands.value, cand_cap))
    nc, nk = min(n, conn_cap), min(n_cands.value, cand_cap)
    return (conns[:nc].copy(), cands[:nk].copy(), tracks[:nc].copy(), pkts[:nk].copy(), seeds[:nc].copy(), peers[:nc].copy(),
            table[:irk_cap].copy(), addrs[:min(n_addrs.value, addr_cap)].copy(), int(n_irks.value), int(n_addrs.value))


def le_crack_identify(words, search_bits, phys_channels, irks=None, tk_limit=LE_PAIR_MAX_TK, key_cap=LE_PAIR_MAX_KEYS, window=8,
                      adv_errors=0, irk_cap=LE_RESOLVE_MAX_IRKS, addr_cap=1 << 16, **kw):
    """le_pair, then le_identify under the short-term keys it recovered, as le_crack composes pairing and decryption: capture in,
    identities out, no key given.  kw: what both take (max_len, min_count, n_streams, pitch_words, n_words, the timing, flags,
    conn_cap, cand_cap, msg_cap, byte_cap, truncate).
    Returns (pair, identities): le_pair's tuple and le_identify's.  When no key was found nothing is raised and identities is None."""
    pair = le_pair(words, search_bits, phys_channels, tk_limit=tk_limit, key_cap=key_cap, adv_errors=adv_errors, **kw)
    found = min(pair[7], key_cap)
    if not found:
        return pair, None
    return pair, le_identify(words, search_bits, phys_channels, pair[6][:found], irks=irks, window=window, adv_errors=adv_errors,
                             irk_cap=irk_cap, addr_cap=addr_cap, **kw)


class DeviceBuffer:
    """A raw HBM allocation owned through the library (no torch needed)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().btbbx_malloc(max(self.nbytes, 8))
        if not self.ptr:
            raise BtbbError("btbbx_malloc(%d): %s" % (nbytes, lib().btbbx_last_error().decode()))

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        check(lib().btbbx_memcpy_h2d(self.ptr, _ptr(a), a.nbytes), "h2d")
        return self

    def download(self, dtype, count):
        out = np.zeros(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib().btbbx_memcpy_d2h(_ptr(out), self.ptr, out.nbytes), "d2h")
        return out

    def zero(self):
        check(lib().btbbx_memset(self.ptr, 0, self.nbytes), "memset")
        return self

    def free(self):
        if self.ptr:
            lib().btbbx_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def packets_to_words(symbol_arrays):
    """List of 0/1 symbol arrays -> (n, 50) packed packet words + lengths (host side packing
    of TEST INPUT only; captured streams are packed on the GPU by btbbx_pack_device)."""
    n = len(symbol_arrays)
    words = np.zeros((n, PKT_WORDS), dtype=np.uint64)
    lengths = np.zeros(n, dtype=np.uint32)
    for i, s in enumerate(symbol_arrays):
        s = np.asarray(s, dtype=np.uint8)[:MAX_SYMBOLS]
        lengths[i] = len(s)
        w = synth.pack_bits(s)
        words[i, :len(w)] = w
    return words, lengths


def run_trials(packet_words, pkt_in):
    """64 clock trials per packet on the GPU -> (n, 64) TRIAL_DTYPE."""
    n = len(packet_words)
    d_pk = DeviceBuffer(packet_words.nbytes).upload(packet_words)
    d_in = DeviceBuffer(pkt_in.nbytes).upload(pkt_in)
    d_tr = DeviceBuffer(n * 64 * 4)
    check(lib().btbbx_trials_device(d_pk.ptr, d_in.ptr, n, d_tr.ptr, None), "btbbx_trials_device")
    check(lib().btbbx_sync(None))
    return d_tr.download(TRIAL_DTYPE, n * 64).reshape(n, 64)


def run_uap_table(packet_words, pkt_in=None):
    """n x 64 uint16: try_clock(c) | type << 8 for every packet and CLK1-6 candidate."""
    packet_words = np.ascontiguousarray(packet_words, dtype=np.uint64)
    n = packet_words.shape[0]
    d_pk = DeviceBuffer(packet_words.nbytes).upload(packet_words)
    d_in = DeviceBuffer(pkt_in.nbytes).upload(pkt_in) if pkt_in is not None else None
    d_out = DeviceBuffer(n * 128)
    try:
        check(lib().btbbx_uap_table_device(d_pk.ptr, d_in.ptr if d_in else None, n, d_out.ptr, None), "btbbx_uap_table_device")
        check(lib().btbbx_sync(None), "sync")
        return d_out.download(np.uint16, n * 64).reshape(n, 64)
    finally:
        d_pk.free()
        d_out.free()
        if d_in:
            d_in.free()


def run_decode(packet_words, pkt_in):
    """decode_header + decode_payload per packet on the GPU -> PKTOUT_DTYPE array."""
    n = len(packet_words)
    d_pk = DeviceBuffer(packet_words.nbytes).upload(packet_words)
    d_in = DeviceBuffer(pkt_in.nbytes).upload(pkt_in)
    d_out = DeviceBuffer(n * PKTOUT_DTYPE.itemsize).zero()
    check(lib().btbbx_decode_device(d_pk.ptr, d_in.ptr, n, d_out.ptr, None), "btbbx_decode_device")
    check(lib().btbbx_sync(None))
    return d_out.download(PKTOUT_DTYPE, n)


def run_decode_hits(stream_words, hits, pkt_in, max_length=MAX_SYMBOLS, via_gather=False, init_out=None, count=None):
    """Decode the packets that start at `hits` (HIT_DTYPE: stream, offset) of the packed streams
    stream_words[n_streams, n_words] -> (PKTOUT_DTYPE array, captured lengths).  via_gather=True takes
    the two-step route (btbbx_gather_packets_device + btbbx_decode_device) for comparison.  init_out: what the
    records hold on entry (a PKTOUT_DTYPE array; zeros if None) -- the decoders leave alone what they do not assign.
    count: the list's length as a word in HBM (btbbx_decode_hits_counted_device, capacity len(hits))."""
    stream_words = np.ascontiguousarray(stream_words, dtype=np.uint64)
    n_streams, n_words = stream_words.shape
    n = len(hits)
    d_w = DeviceBuffer(stream_words.nbytes).upload(stream_words)
    d_h = DeviceBuffer(max(hits.nbytes, 16)).upload(hits)
    d_out = DeviceBuffer(n * PKTOUT_DTYPE.itemsize).zero()
    if init_out is not None:
        d_out.upload(np.ascontiguousarray(init_out, dtype=PKTOUT_DTYPE))
    d_len = DeviceBuffer(n * 4).zero()
    pkt_in = np.array(pkt_in, copy=True)
    d_in = d_pk = None
    try:
        if via_gather:
            d_pk = DeviceBuffer(n * PKT_WORDS * 8).zero()
            check(lib().btbbx_gather_packets_device(d_w.ptr, n_words, n_words, d_h.ptr, n, max_length, d_pk.ptr,
                                                    d_len.ptr, None), "btbbx_gather_packets_device")
            check(lib().btbbx_sync(None))
            lengths = d_len.download(np.uint32, n)
            pkt_in["length"] = lengths
            d_in = DeviceBuffer(pkt_in.nbytes).upload(pkt_in)
            check(lib().btbbx_decode_device(d_pk.ptr, d_in.ptr, n, d_out.ptr, None), "btbbx_decode_device")
        else:
            d_in = DeviceBuffer(pkt_in.nbytes).upload(pkt_in)
            if count is not None:
                d_cnt = DeviceBuffer(8).upload(np.array([count, 0], dtype=np.uint32))
                try:
                    check(lib().btbbx_decode_hits_counted_device(d_w.ptr, n_words, n_words, d_h.ptr, d_in.ptr, d_cnt.ptr, n,
                                                                 max_length, d_out.ptr, d_len.ptr, None),
                          "btbbx_decode_hits_counted_device")
                    check(lib().btbbx_sync(None))
                finally:
                    d_cnt.free()
            else:
                check(lib().btbbx_decode_hits_device(d_w.ptr, n_words, n_words, d_h.ptr, d_in.ptr, n, max_length, d_out.ptr,
                                                     d_len.ptr, None), "btbbx_decode_hits_device")
        check(lib().btbbx_sync(None))
        return d_out.download(PKTOUT_DTYPE, n), d_len.download(np.uint32, n)
    finally:
        for b in (d_w, d_h, d_out, d_len, d_in, d_pk):
            if b is not None:
                b.free()


def _channel_table(channels, n_streams):
    if channels is None:
        return None
    t = np.ascontiguousarray(channels, dtype=np.uint8)
    assert len(t) == n_streams
    return t


def survey(words, search_bits, n_streams=1, pitch_words=None, channels=None, clkn0=0, clk_div=625, clk_phase=0,
           max_ac_errors=2, rec_cap=1 << 20, candidates=False, n_words=None):
    """Every piconet of a capture held in host memory (btbbx_survey_host): scan with LAP_ANY, then UAP / CLK1-6 discovery per
    LAP as the reference's survey mode runs it.  words is (n_streams, pitch_words) or flat; channels = the BR/EDR channel of
    every stream (the stream index when None).  Returns SURVEY_DTYPE records in ascending LAP order -- and, with
    candidates=True, the (n, 64) int16 clock6_candidates as well."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    table = _channel_table(channels, n_streams)
    recs = np.zeros(max(rec_cap, 1), dtype=SURVEY_DTYPE)
    cand = np.zeros((max(rec_cap, 1), 64), dtype=np.int16) if candidates else None
    n = check(lib().btbbx_survey_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, max_ac_errors,
                                      None if table is None else _ptr(table), clkn0, clk_div, clk_phase, _ptr(recs), rec_cap,
                                      None if cand is None else _ptr(cand)), "btbbx_survey_host")
    k = min(n, rec_cap)
    return (recs[:k], cand[:k]) if candidates else recs[:k]


def run_survey_hits(stream_words, hits, entry, channels=None, clk_div=625, clk_phase=0, max_length=MAX_SYMBOLS, count=None,
                    cap=None, rec_cap=None, candidates=True, pitch_words=None, n_words=None):
    """btbbx_survey_hits_device over `hits` (HIT_DTYPE, any order) of the packed streams stream_words[n_streams, pitch_words]
    -> (piconet count, SURVEY_DTYPE records, (n, 64) int16 candidates or None).  entry: one PKTIN_DTYPE record; count: the
    list's length as a word in HBM (None: a NULL d_count); cap / rec_cap default to len(hits)."""
    stream_words = np.ascontiguousarray(stream_words, dtype=np.uint64)
    n_streams, pitch = stream_words.shape
    pitch_words = pitch if pitch_words is None else pitch_words
    n_words = pitch_words if n_words is None else n_words
    cap = len(hits) if cap is None else cap
    rec_cap = cap if rec_cap is None else rec_cap
    table = _channel_table(channels, n_streams)
    entry = np.ascontiguousarray(np.asarray(entry, dtype=PKTIN_DTYPE).reshape(1))
    scratch_bytes = lib().btbbx_survey_scratch_bytes(cap)
    bufs = []

    def dev(nbytes):
        bufs.append(DeviceBuffer(nbytes))
        return bufs[-1]
    try:
        d_w = dev(stream_words.nbytes + 16).upload(stream_words)
        d_h = dev(max(hits.nbytes, 16)).upload(np.ascontiguousarray(hits))
        d_cnt = dev(8).upload(np.array([0 if count is None else count, 0], dtype=np.uint32))
        d_recs = dev(max(rec_cap, 1) * SURVEY_DTYPE.itemsize).zero()
        d_cand = dev(max(rec_cap, 1) * 128).zero() if candidates else None
        d_nrec = dev(8).zero()
        d_scr = dev(scratch_bytes)
        check(lib().btbbx_survey_hits_device(d_w.ptr, n_words, pitch_words, n_streams, d_h.ptr, None if count is None else d_cnt.ptr,
                                             cap, None if table is None else _ptr(table), _ptr(entry), clk_div, clk_phase,
                                             max_length, d_recs.ptr, rec_cap, d_nrec.ptr, d_cand.ptr if candidates else None,
                                             d_scr.ptr, scratch_bytes, None), "btbbx_survey_hits_device")
        check(lib().btbbx_sync(None), "sync")
        n = int(d_nrec.download(np.uint32, 2)[0])
        k = min(n, rec_cap)
        recs = d_recs.download(SURVEY_DTYPE, max(rec_cap, 1))[:k]
        cand = d_cand.download(np.int16, max(rec_cap, 1) * 64).reshape(-1, 64)[:k] if candidates else None
        return n, recs, cand
    finally:
        for b in bufs:
            b.free()


# ---- hop selection / CLK1-27 reversal -------------------------------------------------------
SEQUENCE_LENGTH = 1 << 27


class HopCfg(C.Structure):
    _fields_ = [("address", C.c_uint32), ("afh", C.c_uint8), ("used_channels", C.c_uint8),
                ("reserved", C.c_uint8 * 2), ("bank", C.c_uint8 * 80)]


def hop_cfg(lap, uap, afh_map=None):
    """Kernel configuration of one piconet; afh_map = 10-byte AFH channel map or None."""
    cfg = HopCfg()
    m = None if afh_map is None else np.ascontiguousarray(afh_map, dtype=np.uint8)
    lib().btbbx_hop_cfg_init(C.byref(cfg), ((uap << 24) | lap) & 0xFFFFFFF, None if m is None else _ptr(m))
    return cfg


class ClockJob(C.Structure):
    _fields_ = [("cfg", HopCfg), ("clk6", C.c_uint32), ("aliased", C.c_uint32), ("obs_first", C.c_uint32), ("n_obs", C.c_uint32)]


class ClockResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("n_initial", C.c_uint32), ("stop", C.c_uint32), ("count", C.c_uint32),
                ("cand0", C.c_uint32), ("n_stored", C.c_uint32)]


# one job / one result of the batch reversal (include/btbbx.h btbbx_clock_job / btbbx_clock_result)
HOP_CFG_DTYPE = np.dtype([("address", "<u4"), ("afh", "u1"), ("used_channels", "u1"), ("reserved", "u1", (2,)), ("bank", "u1", (80,))])
CLOCK_JOB_DTYPE = np.dtype([("cfg", HOP_CFG_DTYPE), ("clk6", "<u4"), ("aliased", "<u4"), ("obs_first", "<u4"), ("n_obs", "<u4")])
CLOCK_RESULT_DTYPE = np.dtype([("status", "<u4"), ("n_initial", "<u4"), ("stop", "<u4"), ("count", "<u4"), ("cand0", "<u4"),
                               ("n_stored", "<u4")])
assert CLOCK_JOB_DTYPE.itemsize == C.sizeof(ClockJob) == 104 and CLOCK_RESULT_DTYPE.itemsize == C.sizeof(ClockResult) == 24


def hop_sequence(cfg, first=0, count=SEQUENCE_LENGTH):
    """Channels of CLK1-27 values [first, first+count) as a numpy uint8 array (generated in HBM)."""
    buf = DeviceBuffer(count)
    try:
        check(lib().btbbx_hop_sequence_device(C.byref(cfg), first, count, buf.ptr, None), "btbbx_hop_sequence_device")
        check(lib().btbbx_sync(None), "sync")
        return buf.download(np.uint8, count)
    finally:
        buf.free()


def hop_channels(cfg, clocks):
    clocks = np.ascontiguousarray(clocks, dtype=np.uint32)
    d_in, d_out = DeviceBuffer(clocks.nbytes).upload(clocks), DeviceBuffer(len(clocks))
    try:
        check(lib().btbbx_hop_channels_device(C.byref(cfg), d_in.ptr, len(clocks), d_out.ptr, None),
              "btbbx_hop_channels_device")
        check(lib().btbbx_sync(None), "sync")
        return d_out.download(np.uint8, len(clocks))
    finally:
        d_in.free()
        d_out.free()


class HopReversal:
    """Candidate CLK1-27 values of one piconet, held in HBM (btbbx_hop_reversal_*)."""

    def __init__(self, cfg, clk6, channel, aliased=False):
        n = C.c_int(0)
        self.h = lib().btbbx_hop_reversal_open(C.byref(cfg), clk6, channel, int(aliased), C.byref(n))
        if not self.h:
            raise BtbbError("btbbx_hop_reversal_open: %s" % lib().btbbx_last_error().decode())
        self.count = n.value

    def winnow(self, offsets, channels):
        """Apply observed hops in order; returns (stop, count, first candidate)."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        ch = np.ascontiguousarray(channels, dtype=np.uint8)
        stop, count, cand0 = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().btbbx_hop_reversal_winnow(self.h, _ptr(off), _ptr(ch), len(off), C.byref(stop), C.byref(count),
                                              C.byref(cand0)), "btbbx_hop_reversal_winnow")
        self.count = count.value
        return stop.value, count.value, cand0.value

    def candidates(self):
        out = np.zeros(max(self.count, 1), np.uint32)
        n = lib().btbbx_hop_reversal_candidates(self.h, _ptr(out), len(out))
        check(min(n, 0), "btbbx_hop_reversal_candidates")
        return out[:n]

    def close(self):
        if self.h:
            lib().btbbx_hop_reversal_close(self.h)
            self.h = None


def clock_jobs(cfgs, clk6, observations, aliased=False):
    """The job table and the two shared observation arrays of hop_reversal_batch: (CLOCK_JOB_DTYPE jobs, int32 offsets,
    uint8 channels).  clk6 and aliased are one value for all jobs or one per job; the observations of job j are laid out
    one job after the other."""
    n = len(cfgs)
    assert len(observations) == n
    jobs = np.zeros(n, dtype=CLOCK_JOB_DTYPE)
    jobs["clk6"] = np.broadcast_to(np.asarray(clk6, dtype=np.uint32), (n,))
    jobs["aliased"] = np.broadcast_to(np.asarray(aliased), (n,)).astype(bool)
    offs, chans, at = [], [], 0
    for j, (cfg, (off, ch)) in enumerate(zip(cfgs, observations)):
        jobs["cfg"][j] = np.frombuffer(bytes(cfg), dtype=HOP_CFG_DTYPE)[0]
        off, ch = np.asarray(off, dtype=np.int32).reshape(-1), np.asarray(ch, dtype=np.uint8).reshape(-1)
        assert len(off) == len(ch)
        jobs["obs_first"][j], jobs["n_obs"][j] = at, len(off)
        offs.append(off)
        chans.append(ch)
        at += len(off)
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, dt), dtype=dt)
    return jobs, cat(offs, np.int32), cat(chans, np.uint8)


def hop_reversal_batch_raw(jobs, offsets, channels, cand_cap=0, candidates=None):
    """btbbx_hop_reversal_batch_host over a prepared job table (CLOCK_JOB_DTYPE) and the shared observation arrays ->
    CLOCK_RESULT_DTYPE records, and the (n_jobs, cand_cap) uint32 candidate slots when cand_cap > 0 (`candidates`: their
    initial content, zeros if None; slots no job writes keep it)."""
    jobs = np.ascontiguousarray(jobs, dtype=CLOCK_JOB_DTYPE)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    channels = np.ascontiguousarray(channels, dtype=np.uint8)
    assert len(offsets) == len(channels)
    n = len(jobs)
    results = np.zeros(max(n, 1), dtype=CLOCK_RESULT_DTYPE)
    cand = None
    if cand_cap:
        cand = np.zeros((max(n, 1), cand_cap), np.uint32) if candidates is None else np.ascontiguousarray(candidates, dtype=np.uint32)
        assert cand.size >= n * cand_cap and cand.size % cand_cap == 0
        cand = cand.reshape(-1, cand_cap)
    check(lib().btbbx_hop_reversal_batch_host(_ptr(jobs), n, _ptr(offsets), _ptr(channels), len(offsets), _ptr(results),
                                              None if cand is None else _ptr(cand), cand_cap), "btbbx_hop_reversal_batch_host")
    return (results[:n], cand[:n]) if cand_cap else results[:n]


def hop_reversal_batch(cfgs, clk6, observations, aliased=False, cand_cap=0):
    """CLK1-27 reversal of many piconets in one call (btbbx_hop_reversal_batch_host): job j is the piconet cfgs[j] with
    CLK1-6 clk6[j] at its first observation and the observed hops observations[j] = (offsets, channels); it leaves what
    HopReversal(cfgs[j], clk6[j], channels[0], aliased[j]) and .winnow(offsets, channels) report.  Returns the
    CLOCK_RESULT_DTYPE records -- and, with cand_cap > 0, a list with the first min(count, cand_cap) candidates of every job."""
    jobs, offsets, channels = clock_jobs(cfgs, clk6, observations, aliased)
    if not cand_cap:
        return hop_reversal_batch_raw(jobs, offsets, channels)
    results, cand = hop_reversal_batch_raw(jobs, offsets, channels, cand_cap)
    return results, [cand[j, :int(results["n_stored"][j])].copy() for j in range(len(jobs))]


# ---- clock acquisition from a capture: survey -> job builder -> batch reversal ---------------
JOBS_AFH, JOBS_ALIASED = 1, 2


def run_survey_clock_jobs(stream_words, hits, entry, channels=None, clk_div=625, clk_phase=0, max_length=MAX_SYMBOLS, count=None,
                          flags=0, max_obs=1024, rec_cap=None, job_cap=None, rec_count=True, sentinel=0, pitch_words=None,
                          n_words=None, reversal=False):
    """btbbx_survey_hits_device and btbbx_survey_clock_jobs_device chained on device buffers (the builder reads the survey's
    scratch) -> dict(n_recs, recs, n_jobs, n_obs, jobs, job_rec, offsets, channels, obs_hits): the counts as the device left
    them, every array WHOLE (job_cap jobs, len(hits) observations) over a fill of `sentinel` bytes, so that a caller sees what
    was not written.  rec_count=False hands the builder a NULL d_rec_count.  reversal=True appends
    btbbx_hop_reversal_batch_device with the device's job count and adds `results` (job_cap CLOCK_RESULT_DTYPE records)."""
    stream_words = np.ascontiguousarray(stream_words, dtype=np.uint64)
    n_streams, pitch = stream_words.shape
    pitch_words = pitch if pitch_words is None else pitch_words
    n_words = pitch_words if n_words is None else n_words
    cap = len(hits)
    rec_cap = cap if rec_cap is None else rec_cap
    job_cap = max(rec_cap, 1) if job_cap is None else job_cap
    table = _channel_table(channels, n_streams)
    tp = None if table is None else _ptr(table)
    entry = np.ascontiguousarray(np.asarray(entry, dtype=PKTIN_DTYPE).reshape(1))
    scratch_bytes = lib().btbbx_survey_scratch_bytes(cap)
    bufs = []

    def dev(nbytes, fill=None):
        bufs.append(DeviceBuffer(nbytes))
        if fill is not None:
            check(lib().btbbx_memset(bufs[-1].ptr, fill, max(nbytes, 8)), "memset")
        return bufs[-1]
    try:
        d_w = dev(stream_words.nbytes + 16).upload(stream_words)
        d_h = dev(max(hits.nbytes, 16)).upload(np.ascontiguousarray(hits))
        d_cnt = dev(8).upload(np.array([0 if count is None else count, 0], dtype=np.uint32))
        d_recs = dev(max(rec_cap, 1) * SURVEY_DTYPE.itemsize, 0)
        d_nrec = dev(8, 0)
        d_scr = dev(scratch_bytes)
        d_jobs = dev(job_cap * CLOCK_JOB_DTYPE.itemsize, sentinel)
        d_jrec = dev(job_cap * 4, sentinel)
        d_off, d_ch, d_oh = dev(max(cap, 1) * 4, sentinel), dev(max(cap, 1), sentinel), dev(max(cap, 1) * 4, sentinel)
        d_n = dev(8, sentinel)
        check(lib().btbbx_survey_hits_device(d_w.ptr, n_words, pitch_words, n_streams, d_h.ptr, None if count is None else d_cnt.ptr,
                                             cap, tp, _ptr(entry), clk_div, clk_phase, max_length, d_recs.ptr, rec_cap, d_nrec.ptr,
                                             None, d_scr.ptr, scratch_bytes, None), "btbbx_survey_hits_device")
        check(lib().btbbx_survey_clock_jobs_device(d_recs.ptr, d_nrec.ptr if rec_count else None, rec_cap, d_scr.ptr, scratch_bytes, cap,
                                                   tp, n_streams, flags, max_obs, d_jobs.ptr, job_cap, d_n.ptr, d_jrec.ptr, d_off.ptr,
                                                   d_ch.ptr, d_oh.ptr, cap, d_n.ptr + 4, None), "btbbx_survey_clock_jobs_device")
        out = {}
        if reversal:
            sb = lib().btbbx_hop_reversal_batch_scratch_bytes(job_cap, 0)
            d_bs, d_res = dev(sb), dev(job_cap * CLOCK_RESULT_DTYPE.itemsize, sentinel)
            check(lib().btbbx_hop_reversal_batch_device(d_jobs.ptr, d_n.ptr, job_cap, d_off.ptr, d_ch.ptr, cap, d_res.ptr, None, 0,
                                                        d_bs.ptr, sb, None), "btbbx_hop_reversal_batch_device")
        check(lib().btbbx_sync(None), "sync")
        if reversal:
            out["results"] = d_res.download(CLOCK_RESULT_DTYPE, job_cap)
        n_recs = int(d_nrec.download(np.uint32, 2)[0])
        n_jobs, n_obs = (int(x) for x in d_n.download(np.uint32, 2))
        out.update(n_recs=n_recs, recs=d_recs.download(SURVEY_DTYPE, max(rec_cap, 1))[:min(n_recs, rec_cap)], n_jobs=n_jobs, n_obs=n_obs,
                   jobs=d_jobs.download(CLOCK_JOB_DTYPE, job_cap), job_rec=d_jrec.download(np.uint32, job_cap),
                   offsets=d_off.download(np.int32, max(cap, 1)), channels=d_ch.download(np.uint8, max(cap, 1)),
                   obs_hits=d_oh.download(np.uint32, max(cap, 1)))
        return out
    finally:
        for b in bufs:
            b.free()


def acquire(words, search_bits, n_streams=1, pitch_words=None, channels=None, clkn0=0, clk_div=625, clk_phase=0, afh=False,
            aliased=False, max_obs=1024, cand_cap=0, max_ac_errors=2, rec_cap=1 << 20, n_words=None):
    """Capture in, (LAP, UAP, CLK1-27) of every piconet out (btbbx_acquire_host): survey() and, for every settled piconet, the
    CLK1-27 reversal over its packets from the settling run on.  Returns (SURVEY_DTYPE records in ascending LAP order, job_rec =
    the record index of every job, CLOCK_RESULT_DTYPE records) -- and, with cand_cap > 0, a list with the first min(count,
    cand_cap) candidates of every job.  A result with count == 1 has CLK1-27 of its run's first packet in cand0."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    table = _channel_table(channels, n_streams)
    k = max(rec_cap, 1)
    recs = np.zeros(k, dtype=SURVEY_DTYPE)
    job_rec, results = np.zeros(k, np.uint32), np.zeros(k, dtype=CLOCK_RESULT_DTYPE)
    cand = np.zeros((k, cand_cap), np.uint32) if cand_cap else None
    n_jobs = C.c_uint64(0)
    flags = (JOBS_AFH if afh else 0) | (JOBS_ALIASED if aliased else 0)
    n = check(lib().btbbx_acquire_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, max_ac_errors,
                                       None if table is None else _ptr(table), clkn0, clk_div, clk_phase, _ptr(recs), rec_cap, None,
                                       flags, max_obs, None, _ptr(job_rec), _ptr(results), rec_cap, C.byref(n_jobs),
                                       None if cand is None else _ptr(cand), cand_cap), "btbbx_acquire_host")
    nj = min(n_jobs.value, rec_cap)
    out = (recs[:min(n, rec_cap)], job_rec[:nj], results[:nj])
    if cand_cap:
        out += ([cand[j, :int(results["n_stored"][j])].copy() for j in range(nj)],)
    return out


# ---- following: every packet of every acquired piconet with its own UAP and clock ---------------
NO_PICONET = 0xFFFFFFFF


def run_follow_hits(stream_words, hits, entry, channels=None, clk_div=625, clk_phase=0, max_length=MAX_SYMBOLS, count=None, flags=0,
                    max_obs=1024, sentinel=0, pitch_words=None, n_words=None, recs=None, rec_count="device", rec_cap=None, jobs=None,
                    job_rec=None, results=None, n_jobs="device", job_cap=None, follow_channels="same", follow_hits=None,
                    follow_count="same", lengths=True, zero_out=0):
    """btbbx_follow_hits_device chained behind the calls of run_survey_clock_jobs(..., reversal=True) on device buffers ->
    dict(n_recs, recs, n_jobs, jobs, job_rec, results = the tables the follow read; pkt_in, follow, pkt_out, lengths, sums = its
    outputs), every output array WHOLE (one entry per hit, rec_cap sums) over a fill of `sentinel` bytes.  The first zero_out
    records of d_out are zeroed instead: the decoders read what a record holds on entry as the packet's earlier state.
    The follow's inputs can be replaced (tests hand it doctored tables): recs / jobs / job_rec / results = arrays uploaded in
    place of what the chain left; rec_count / n_jobs = "device" (the chain's count), None (a NULL pointer) or a number put into
    HBM; rec_cap / job_cap = the caps given to the follow (job_cap = 0 passes NULL job pointers); follow_channels = the channel
    table of the follow alone; follow_hits / follow_count = another list (same capture) and its count for the follow alone
    (follow_count: "same" = `count`, None = NULL, or a number)."""
    stream_words = np.ascontiguousarray(stream_words, dtype=np.uint64)
    n_streams, pitch = stream_words.shape
    pitch_words = pitch if pitch_words is None else pitch_words
    n_words = pitch_words if n_words is None else n_words
    cap = len(hits)
    table = _channel_table(channels, n_streams)
    tp = None if table is None else _ptr(table)
    ftable = table if isinstance(follow_channels, str) else _channel_table(follow_channels, n_streams)
    ftp = None if ftable is None else _ptr(ftable)
    entry = np.ascontiguousarray(np.asarray(entry, dtype=PKTIN_DTYPE).reshape(1))
    scratch_bytes = lib().btbbx_survey_scratch_bytes(cap)
    chain_recs, chain_jobs = max(cap, 1), max(cap, 1)
    bufs = []

    def dev(nbytes, fill=None):
        bufs.append(DeviceBuffer(nbytes))
        if fill is not None:
            check(lib().btbbx_memset(bufs[-1].ptr, fill, max(nbytes, 8)), "memset")
        return bufs[-1]

    def table_of(given, d_chain, dtype):
        if given is None:
            return d_chain
        given = np.ascontiguousarray(given, dtype=dtype)
        return dev(max(given.nbytes, 8), 0).upload(given)

    def count_of(given, d_chain):
        if given is None:
            return None
        if isinstance(given, str):
            return d_chain.ptr
        return dev(8).upload(np.array([given, 0], dtype=np.uint32)).ptr
    try:
        d_w = dev(stream_words.nbytes + 16).upload(stream_words)
        d_h = dev(max(hits.nbytes, 16)).upload(np.ascontiguousarray(hits))
        d_cnt = dev(8).upload(np.array([0 if count is None else count, 0], dtype=np.uint32))
        d_recs, d_nrec, d_scr = dev(chain_recs * SURVEY_DTYPE.itemsize, 0), dev(8, 0), dev(scratch_bytes)
        d_jobs, d_jrec = dev(chain_jobs * CLOCK_JOB_DTYPE.itemsize, 0), dev(chain_jobs * 4, 0)
        d_off, d_ch, d_n = dev(max(cap, 1) * 4, 0), dev(max(cap, 1), 0), dev(8, 0)
        sb = lib().btbbx_hop_reversal_batch_scratch_bytes(chain_jobs, 0)
        d_bs, d_res = dev(sb), dev(chain_jobs * CLOCK_RESULT_DTYPE.itemsize, 0)
        check(lib().btbbx_survey_hits_device(d_w.ptr, n_words, pitch_words, n_streams, d_h.ptr, None if count is None else d_cnt.ptr,
                                             cap, tp, _ptr(entry), clk_div, clk_phase, max_length, d_recs.ptr, chain_recs, d_nrec.ptr,
                                             None, d_scr.ptr, scratch_bytes, None), "btbbx_survey_hits_device")
        check(lib().btbbx_survey_clock_jobs_device(d_recs.ptr, d_nrec.ptr, chain_recs, d_scr.ptr, scratch_bytes, cap, tp, n_streams, flags,
                                                   max_obs, d_jobs.ptr, chain_jobs, d_n.ptr, d_jrec.ptr, d_off.ptr, d_ch.ptr, None, cap,
                                                   d_n.ptr + 4, None), "btbbx_survey_clock_jobs_device")
        check(lib().btbbx_hop_reversal_batch_device(d_jobs.ptr, d_n.ptr, chain_jobs, d_off.ptr, d_ch.ptr, cap, d_res.ptr, None, 0, d_bs.ptr,
                                                    sb, None), "btbbx_hop_reversal_batch_device")
        # the follow's own view of the tables
        f_recs, f_jobs = table_of(recs, d_recs, SURVEY_DTYPE), table_of(jobs, d_jobs, CLOCK_JOB_DTYPE)
        f_jrec, f_res = table_of(job_rec, d_jrec, np.uint32), table_of(results, d_res, CLOCK_RESULT_DTYPE)
        f_rec_cap = (chain_recs if recs is None else max(len(recs), 1)) if rec_cap is None else rec_cap
        f_job_cap = (chain_jobs if jobs is None and job_rec is None and results is None else
                     min(len(x) for x in (jobs, job_rec, results) if x is not None)) if job_cap is None else job_cap
        fh = hits if follow_hits is None else np.ascontiguousarray(follow_hits, dtype=HIT_DTYPE)
        f_cap = len(fh)
        d_fh = d_h if follow_hits is None else dev(max(fh.nbytes, 16)).upload(fh)
        f_count = (None if count is None else d_cnt.ptr) if isinstance(follow_count, str) else count_of(follow_count, None)
        d_in, d_fol = dev(f_cap * PKTIN_DTYPE.itemsize, sentinel), dev(f_cap * FOLLOW_PKT_DTYPE.itemsize, sentinel)
        d_out, d_len = dev(f_cap * PKTOUT_DTYPE.itemsize, sentinel), dev(f_cap * 4, sentinel)
        d_sums = dev(max(f_rec_cap, 1) * FOLLOW_SUM_DTYPE.itemsize, sentinel)
        if zero_out:
            check(lib().btbbx_memset(d_out.ptr, 0, min(zero_out, f_cap) * PKTOUT_DTYPE.itemsize), "memset")
        no_jobs = f_job_cap == 0
        check(lib().btbbx_follow_hits_device(d_w.ptr, n_words, pitch_words, n_streams, d_fh.ptr, f_count, f_cap, f_recs.ptr,
                                             count_of(rec_count, d_nrec), f_rec_cap, None if no_jobs else f_jobs.ptr,
                                             None if no_jobs else f_jrec.ptr, None if no_jobs else f_res.ptr,
                                             None if no_jobs else count_of(n_jobs, d_n), f_job_cap, ftp, _ptr(entry), clk_div, clk_phase,
                                             max_length, d_in.ptr, d_fol.ptr, d_out.ptr, d_len.ptr if lengths else None, d_sums.ptr, None),
              "btbbx_follow_hits_device")
        check(lib().btbbx_sync(None), "sync")
        n_recs = int(d_nrec.download(np.uint32, 2)[0])
        nj = int(d_n.download(np.uint32, 2)[0])
        return dict(n_recs=n_recs, recs=d_recs.download(SURVEY_DTYPE, chain_recs)[:min(n_recs, chain_recs)], n_jobs=nj,
                    jobs=d_jobs.download(CLOCK_JOB_DTYPE, chain_jobs)[:nj], job_rec=d_jrec.download(np.uint32, chain_jobs)[:nj],
                    results=d_res.download(CLOCK_RESULT_DTYPE, chain_jobs)[:nj],
                    pkt_in=d_in.download(PKTIN_DTYPE, f_cap), follow=d_fol.download(FOLLOW_PKT_DTYPE, f_cap),
                    pkt_out=d_out.download(PKTOUT_DTYPE, f_cap), lengths=d_len.download(np.uint32, f_cap),
                    sums=d_sums.download(FOLLOW_SUM_DTYPE, max(f_rec_cap, 1)))
    finally:
        for b in bufs:
            b.free()


def follow(words, search_bits, n_streams=1, pitch_words=None, channels=None, clkn0=0, clk_div=625, clk_phase=0, afh=False,
           aliased=False, max_obs=1024, max_ac_errors=2, rec_cap=1 << 16, hit_cap=1 << 16, packets=True, n_words=None):
    """Capture in, every packet of every piconet decoded with its piconet's UAP and clock (btbbx_follow_host): acquire() and,
    behind it, the FOLLOWING stage over the same ordered hit list.  Returns dict(recs, job_rec, results as acquire() returns
    them; n_hits = all hits; hits / follow / pkts = the first min(n_hits, hit_cap) in (stream, offset) order (pkts None with
    packets=False); sums = one FOLLOW_SUM_DTYPE per record, over all hits)."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if pitch_words is None:
        pitch_words = len(words) // n_streams
    if n_words is None:
        n_words = pitch_words
    assert n_words <= pitch_words and (n_streams - 1) * pitch_words + n_words <= len(words)
    table = _channel_table(channels, n_streams)
    k, hk = max(rec_cap, 1), max(hit_cap, 1)
    recs, sums = np.zeros(k, dtype=SURVEY_DTYPE), np.zeros(k, dtype=FOLLOW_SUM_DTYPE)
    job_rec, results = np.zeros(k, np.uint32), np.zeros(k, dtype=CLOCK_RESULT_DTYPE)
    hits, fol = np.zeros(hk, dtype=HIT_DTYPE), np.zeros(hk, dtype=FOLLOW_PKT_DTYPE)
    pkts = np.zeros(hk, dtype=PKTOUT_DTYPE) if packets else None
    n_jobs, n_hits = C.c_uint64(0), C.c_uint64(0)
    flags = (JOBS_AFH if afh else 0) | (JOBS_ALIASED if aliased else 0)
    n = check(lib().btbbx_follow_host(_ptr(words), n_words, pitch_words, n_streams, search_bits, max_ac_errors,
                                      None if table is None else _ptr(table), clkn0, clk_div, clk_phase, _ptr(recs), rec_cap, flags,
                                      max_obs, _ptr(job_rec), _ptr(results), rec_cap, C.byref(n_jobs), _ptr(hits), _ptr(fol),
                                      None if pkts is None else _ptr(pkts), hit_cap, C.byref(n_hits), _ptr(sums)), "btbbx_follow_host")
    nr, nj, nh = min(n, rec_cap), min(n_jobs.value, rec_cap), min(n_hits.value, hit_cap)
    return dict(recs=recs[:nr], job_rec=job_rec[:nj], results=results[:nj], n_hits=n_hits.value, hits=hits[:nh], follow=fol[:nh],
                pkts=None if pkts is None else pkts[:nh], sums=sums[:nr])
