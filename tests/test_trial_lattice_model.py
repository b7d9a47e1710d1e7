"""The packet lattice of tests/_trial_lattice.py sits on the boundaries it is named for, and the oracle's
64-clock tables of it equal the compiled reference's (CPU only).  tests/test_gpu_trial_lattice.py holds
the kernels against these tables; a lattice that drifted off its boundaries would make that comparison
weaker without failing it, so the drift is caught here."""
import ctypes as C
from collections import Counter, defaultdict

import numpy as np
import pytest

import _libs
import _trial_lattice as tl
from libbtbb_amd import synth

DM = ("DM1", "DM3", "DM5", "DV")
DH = ("DH1", "DH3", "DH5")
TYPE_OF = {v: k for k, v in tl.NAMES.items()}
TYPE_OF[tl.HV3_AS] = 7


@pytest.fixture(scope="module")
def lat():
    return tl.lattice()


@pytest.fixture(scope="module")
def tables():
    return tl.tables()


def _plain(lat, i):
    """Whitened on air, the entry's WHITENED flag says so, header untouched."""
    return bool(lat.air_white[i]) and int(lat.pin["flags"][i]) & 1 == 1 and not lat.tags[i][1].startswith("hdr")


def test_lattice_covers_every_length_cut_and_entry_state(lat):
    n = len(lat.syms)
    assert 10000 <= n <= 30000, n
    assert all(0 < len(s) <= 3125 for s in lat.syms)
    assert lat.words.shape == (n, 50) and (lat.pin["length"] == [len(s) for s in lat.syms]).all()
    full = defaultdict(set)
    kinds = defaultdict(set)
    for name, bnd, L in lat.tags:
        kinds[name].update(bnd.split(":")[-1].split("+"))
        if bnd == "full":
            full[name].add(L)
    for t, m in tl.MAXBODY.items():
        assert set(range(m + 1)) <= full[tl.NAMES[t]], tl.NAMES[t]
    for name in DM + DH:
        t = TYPE_OF[name]
        over = tl.REF_CAP[t] - (4 if t in tl.TWO_BYTE else 3) + 1
        assert (name, "field_max", over - 1) in set(lat.tags) and (name, "field_max+1:full", over) in set(lat.tags), name
        assert {"ph_end", "ph_end-1", "bitlen", "bitlen-1"} <= kinds[name], name
    for name in DM + ("FHS", "HV2", "EV4"):
        assert {"fec_clean", "fec@first", "fec@last-1", "fec@last", "fec@after"} <= kinds[name], name
    assert {"ev4_need", "ev4_need-1", "reg1_zero"} <= kinds["EV4"]
    for name in TYPE_OF:
        assert {"full", "end", "end-1", "122", "121", "3125", "hdr3_right", "hdr3_wrong", "hdr4_right",
                "hdr4_wrong"} <= kinds[name], name
        assert any(b.startswith("nowh") for nm, b, _ in lat.tags if nm == name), name
    assert (np.array([len(s) for s in lat.syms]) == 3125).sum() >= 1000
    assert set(lat.pin["type"]) == set(tl.ENTRY_TYPES)
    assert set(lat.pin["llid"]) == {0, 1, 2, 3} and set(lat.pin["flow"]) == {0, 1}
    white = (lat.pin["flags"] & 1).astype(bool)
    assert (white != lat.air_white).sum() > 500 and (~lat.air_white & ~white).sum() > 100
    for bit in (tl.F_UAP_VALID, tl.F_CLK6_VALID, tl.F_HAS_PAYLOAD):
        assert 0.3 < ((lat.pin["flags"] & bit) != 0).mean() < 0.7


def test_trial_table_helper_equals_the_loop(lat):
    """orc_trial_table against try_clock / crc_check called one clock at a time from Python (the form of
    _oracle_trials in test_gpu_packets.py), entry state included: a packet of every kind and every 53rd."""
    orc = _libs.oracle()
    first = {}
    for i, (name, bnd, _) in enumerate(lat.tags):
        first.setdefault((name, bnd), i)
    sample = sorted(set(first.values()) | set(range(0, len(lat.syms), 53)))
    for i in sample:
        s, e = lat.syms[i], lat.pin[i]
        p = orc.orc_packet_new()
        orc.orc_packet_init_found(p, 0, 0)
        orc.orc_packet_set_data(p, _libs.ptr(s), len(s), 0, 0)
        p.contents.flags = int(e["flags"])
        p.contents.payload_llid, p.contents.payload_flow = int(e["llid"]), int(e["flow"])
        want = []
        for clock in range(64):
            p.contents.packet_type, p.contents.UAP = int(e["type"]), int(e["uap"])
            u = orc.orc_try_clock(clock, p)
            rv = orc.orc_crc_check(clock, p)
            want.append((u, p.contents.packet_type, rv))
        orc.orc_packet_free(p)
        got = tl.oracle_table(orc, s, e)
        assert [(int(t["uap"]), int(t["type"]), int(t["rv"])) for t in got] == want, lat.tags[i]


def test_verdicts_at_the_true_clock(lat, tables):
    """Every packet on its boundary: the verdict at the clock it was built with is the one the reference's check
    gives on that side of it (bluetooth_packet.c: DM :898-958, DH :962-1011, EV4 :1044-1097, HV :1131-1174,
    fhs :783-818, the crc_check mapping :708-769)."""
    seen = Counter()
    # EV4 packets whose CRC register happens to be zero in front of the CRC (then every cut behind that says 10)
    early = {L for i, (nm, b, L) in enumerate(lat.tags)
             if nm == "EV4" and b == "end-1" and _plain(lat, i) and int(tables[i, lat.clk6[i]]["rv"]) == 10}
    assert len(early) <= 2, early
    for i, (name, bnd, L) in enumerate(lat.tags):
        if not _plain(lat, i):
            continue
        tr = tables[i, int(lat.clk6[i])]
        u, ty, rv = int(tr["uap"]), int(tr["type"]), int(tr["rv"])
        assert (u, ty) == (int(lat.uap[i]), TYPE_OF[name]), (lat.tags[i], u, ty)
        if bnd.startswith("field_max+1:"):
            assert rv != 10, lat.tags[i]                          # the length is clamped: the CRC is not where it was put
            continue
        cuts = set(bnd.split("+"))
        dm1_zero = 0 if name == "DM1" else 1                      # a failing DM1 / FHS / HV1 keeps its 0 (:760-768)
        want = None
        if name in DM + DH:
            if cuts & {"full", "3125", "end", "fec_clean", "fec@after", "field_max", "bitlen"} and \
                    not (name in DM and "bitlen" in cuts):
                want = 10
            elif name in DM and "end-1" in cuts:
                want = 10                                         # the last symbol is a parity bit: read as 0, corrected
            elif cuts & {"bitlen-1", "ph_end"}:
                want = 1                                          # bitlength > size
            elif cuts & {"fec@first", "fec@last-1", "fec@last"}:
                want = dm1_zero if name in DM else None
            elif cuts & {"ph_end-1", "122", "121"}:
                want = dm1_zero if name in DM else 1
        elif name == "FHS":
            want = 1000 if cuts & {"full", "3125", "end", "fec_clean", "fec@after"} else \
                1 if cuts & {"end-1", "122", "121"} else 0 if cuts & {"fec@first", "fec@last-1", "fec@last"} else None
        elif name == "HV1":
            want = 2 if cuts & {"full", "3125", "end"} else 1 if cuts & {"end-1", "122", "121"} else None
        elif name == "EV4":
            if L == 120:                                          # 98 blocks are all the loop looks at
                want = 2 if cuts & {"ev4_need", "fec_clean", "end", "fec@after"} else None
            elif cuts & {"ev4_need", "fec_clean"}:
                want = 10
            elif "reg1_zero" in cuts or L not in early and cuts & {"ev4_need-1", "end", "end-1", "fec@first",
                                                                  "fec@last-1", "fec@last", "fec@after", "122", "121"}:
                want = 1                                          # the CRC is tested one block late (:1082)
        else:                                                     # AUX1, EV3, EV5, HV2, HV3, NULL, POLL: always 1
            want = 1
        if want is not None:
            assert rv == want, (lat.tags[i], rv, want)
            seen[(name, want)] += 1
    assert seen[("DM3", 10)] > 300 and seen[("DH5", 1)] > 900 and seen[("EV4", 10)] > 200 and seen[("FHS", 0)] > 100
    assert seen[("DM1", 0)] > 50 and seen[("HV1", 2)] > 50 and seen[("FHS", 1000)] > 150


def test_header_fec_boundary(lat, tables):
    """unfec13 (:552-568) passes up to 3 disagreeing triples and fails at 4, whatever the majority says; a wrong
    majority is a wrong header bit, which the HEC always notices (a different UAP at the true clock)."""
    ok = tl.header_fec_ok()
    n = Counter()
    for i, (name, bnd, L) in enumerate(lat.tags):
        if not bnd.startswith("hdr"):
            continue
        e, tr = lat.pin[i], tables[i]
        c = int(lat.clk6[i])
        if bnd.startswith("hdr4"):
            assert not ok[i], lat.tags[i]
            assert (tr["uap"] == 0).all() and (tr["type"] == e["type"]).all(), lat.tags[i]
        else:
            assert ok[i], lat.tags[i]
            if int(e["flags"]) & 1:
                right = int(tr[c]["uap"]) == int(lat.uap[i]) and int(tr[c]["type"]) == TYPE_OF[name]
                assert right == bnd.endswith("right"), lat.tags[i]
        n[bnd] += 1
    assert min(n.values()) >= 40 and len(n) == 4, n
    # a failing header with the packet's own type and UAP on entry: crc_check still decodes the payload
    own = [i for i, t in enumerate(lat.tags) if t[1] == "hdr4_right" and int(lat.pin["uap"][i]) == int(lat.uap[i])
           and int(lat.pin["type"][i]) == TYPE_OF[t[0]] and t[0] in DM + DH and int(lat.pin["flags"][i]) & 1]
    assert sum(int(tables[i, lat.clk6[i]]["rv"]) == 10 for i in own) >= 5


def test_unwhitened_packets_do_not_depend_on_the_clock(lat, tables):
    """A packet sent without whitening, its flag cleared: one header, one payload for all 64 clocks."""
    count = 0
    for i, (name, bnd, L) in enumerate(lat.tags):
        if lat.air_white[i] or int(lat.pin["flags"][i]) & 1:
            continue
        tr = tables[i]
        assert (tr == tr[0]).all(), lat.tags[i]
        assert int(tr[0]["uap"]) == int(lat.uap[i]) and int(tr[0]["type"]) == TYPE_OF[name], lat.tags[i]
        if bnd == "nowh:full":
            want = {"FHS": 1000, "HV1": 2}.get(name, 10 if name in DM + DH else None)
            if want is not None:
                assert int(tr[0]["rv"]) == want, lat.tags[i]
                count += 1
    assert count >= 30


def test_reg1_zero_packets_zero_the_register_after_one_byte(lat, tables):
    """The EV4 packets for the kernel's `from two bytes on`: at the true clock the UAP is 0 (CRC seed 0) and the
    first payload byte decodes to 0, so the register is 0 after one byte -- which the reference does not count."""
    orc = _libs.oracle()
    idx = [i for i, t in enumerate(lat.tags) if t[1] == "reg1_zero" and _plain(lat, i)]
    assert len(idx) >= 60
    buf = np.zeros(10, np.uint8)
    for i in idx:
        c = int(lat.clk6[i])
        s = lat.syms[i]
        assert orc.orc_unfec23(_libs.ptr(np.ascontiguousarray(s[122:137])), 10, _libs.ptr(buf))
        first = buf[:8] ^ synth.whitening(c, 18, 8)
        assert int(tables[i, c]["uap"]) == 0 and not first.any()
        assert int(tables[i, c]["rv"]) == 1, lat.tags[i]


def test_oracle_tables_equal_the_compiled_reference(lat, tables):
    """try_clock / crc_check of the unmodified reference, one packet object per packet, the entry's type and UAP
    put back before every clock as orc_trial_table does: every kind of packet and every 5th of the lattice."""
    ref = _libs.ref()
    if ref is None:
        pytest.skip("compiled reference not available")
    first = {}
    for i, (name, bnd, _) in enumerate(lat.tags):
        first.setdefault((name, bnd), []).append(i)
    sample = sorted({j for v in first.values() for j in v[:3]} | set(range(0, len(lat.syms), 5)))
    p = C.c_void_p(ref.btbb_packet_new())
    view = _libs.RefPacketView(ref, p.value)
    off = {f: view._off(f) for f in ("LAP", "ac_errors", "flags", "UAP", "packet_type", "payload_llid", "payload_flow")}
    ref.btbb_packet_unref(p)
    bad = []
    for i in sample:
        s, e = lat.syms[i], lat.pin[i]
        p = C.c_void_p(ref.btbb_packet_new())
        a = p.value
        C.c_uint32.from_address(a + off["LAP"]).value = 0
        C.c_uint8.from_address(a + off["ac_errors"]).value = 0
        ref.btbb_packet_set_data(p, _libs.ptr(s), len(s), 0, 0)
        C.c_uint32.from_address(a + off["flags"]).value = int(e["flags"])
        C.c_uint8.from_address(a + off["payload_llid"]).value = int(e["llid"])
        C.c_uint8.from_address(a + off["payload_flow"]).value = int(e["flow"])
        ty = C.c_uint8.from_address(a + off["packet_type"])
        ua = C.c_uint8.from_address(a + off["UAP"])
        got = []
        for clock in range(64):
            ty.value, ua.value = int(e["type"]), int(e["uap"])
            u = ref.try_clock(clock, p)
            rv = ref.crc_check(clock, p)
            got.append((u, ty.value, rv))
        ref.btbb_packet_unref(p)
        want = [(int(t["uap"]), int(t["type"]), int(t["rv"])) for t in tables[i]]
        if got != want:
            bad.append((lat.tags[i], [(c, got[c], want[c]) for c in range(64) if got[c] != want[c]][:3]))
    assert not bad, (len(bad), bad[:5])
    assert len(sample) > 3000
