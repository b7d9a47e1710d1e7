"""LE data extraction (libbtbb_amd/csrc/le_data.h) on the GPU over the worlds of tests/_le_data_lattice.py: every short sequence of
member states, the gather's product of source residue, destination residue and length, the streams' end at every distance, and more
than 2^32 octets.  Everything is held against the model (the far world: against closed forms that tests/test_le_data_lattice_model.py
holds against the model) byte for byte, with the 0xA5 guards of tests/test_gpu_le_data.py behind the records, behind the stored
prefix of the octets, behind the scratch and in the counts."""
import time

import numpy as np
import pytest

import _le_data as dm
import _le_data_lattice as dl
import libbtbb_amd as bt
from test_gpu_le_data import _check, _filled, _same
from test_le_data_lattice_model import sequence_caps

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE
DATA, DPKT, MSG = bt.LE_DATA_DTYPE, bt.LE_DATA_PKT_DTYPE, bt.LE_MSG_DTYPE


@pytest.fixture(scope="module", autouse=True)
def _init():
    import torch                                            # (a torch that does not import fails these tests, it does not skip them)
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


# ---- A -----------------------------------------------------------------------------------------------------------------------------
def test_the_sequence_world():
    b, want = dl.sequence_world(), dl.sequence_model()
    assert len(b.cands) % 2048 and len(b.conns) % 256
    _check(b, want=want)


def test_the_sequence_world_under_caps():
    b = dl.sequence_world()
    caps = sequence_caps(dl.sequence_model())
    want = dl.sequence_model(None, *caps)
    assert 0 < len(want.payload) < caps[1] and len(want.msgs) == caps[0]
    _check(b, *caps, want=want)


# ---- B -----------------------------------------------------------------------------------------------------------------------------
def test_the_product_lattice():
    want = _check(dl.product_list())
    assert want.n_msgs == 15360 + 64 * 37


@pytest.mark.parametrize("pad", [0, 1])
def test_the_end_lattice(pad):
    b = dl.end_list(pad)
    assert np.asarray(b.words).shape[1] == b.n_words + pad
    _check(b)


# ---- C -----------------------------------------------------------------------------------------------------------------------------
def _upload(a):
    import torch
    a = np.ascontiguousarray(a)
    raw = (a if a.flags.writeable else a.copy()).view(np.uint8).reshape(-1)
    pad = (-len(raw)) % 8
    return torch.from_numpy(np.concatenate([raw, np.zeros(pad, np.uint8)]) if pad else raw).cuda()


class _Far:
    """The far world on the device: one upload, any number of calls."""

    def __init__(self, w):
        import torch
        self.w, self.n, self.k = w, len(w.cands), len(w.conns)
        self.fixed = dl.far_fixed(w, (DATA, DPKT))
        self.d_cands, self.d_conns, self.d_pkts, self.d_words = _upload(w.cands), _upload(w.conns), _upload(w.pkts), _upload(w.words)
        self.d_phys, self.d_tracks = _upload(np.asarray(dm.MHZ, np.uint16)), _filled(self.k * TRACK.itemsize)
        self.d_cnt = torch.from_numpy(np.array([self.n, self.k], np.uint32).view(np.int32)).cuda()
        self.scratch = bt.lib().btbbx_le_data_scratch_bytes(self.n, self.k)
        self.d_scr = _filled(self.scratch)

    def call(self, msg_cap, byte_cap):
        """-> (data, dpkts, msgs with one record of guard, the octets' device buffer with 64 guard octets, n_msgs, n_bytes)"""
        import torch
        w = self.w
        d_data, d_dpkts = _filled((self.k + 1) * DATA.itemsize), _filled((self.n + 1) * DPKT.itemsize)
        d_msgs, d_bytes, d_counts = _filled((msg_cap + 1) * MSG.itemsize), _filled(byte_cap + 64), _filled(16)
        p = self.d_cnt.data_ptr()
        bt.check(bt.lib().btbbx_le_data_device(self.d_words.data_ptr(), w.n_words, w.words.shape[1], w.words.shape[0], self.d_phys.data_ptr(),
                                               self.d_cands.data_ptr(), p, self.n, self.d_conns.data_ptr(), p + 4, self.k,
                                               self.d_tracks.data_ptr(), self.d_pkts.data_ptr(), d_data.data_ptr(), d_dpkts.data_ptr(),
                                               d_msgs.data_ptr() if msg_cap else None, msg_cap, d_counts.data_ptr() + 8,
                                               d_bytes.data_ptr() if byte_cap else None, byte_cap, d_counts.data_ptr(),
                                               self.d_scr.data_ptr(), self.scratch, None), "btbbx_le_data_device")
        torch.cuda.synchronize()
        assert bool((self.d_scr[self.scratch:] == 0xA5).all())                     # nothing behind the scratch
        counts = d_counts.cpu().numpy()
        assert counts[12:].tobytes() == b"\xa5" * (len(counts) - 12)
        rec = lambda buf, n, t: buf.cpu().numpy()[:n * t.itemsize].view(t)         # noqa: E731
        return (rec(d_data, self.k + 1, DATA), rec(d_dpkts, self.n + 1, DPKT), rec(d_msgs, msg_cap + 1, MSG), d_bytes,
                int(counts[8:12].view(np.uint32)[0]), int(counts[:8].view(np.uint64)[0]))


def _same_records(got, want, what):
    """_same for millions of records: numpy finds the first that differs."""
    kept = len(want)
    size = want.dtype.itemsize
    a, b = got[:kept].view(np.uint8).reshape(kept, size), want.view(np.uint8).reshape(kept, size)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert not len(bad), "%s %d: %s, closed form %s (%d of %d differ)" % (what, bad[0], got[bad[0]], want[bad[0]], len(bad), kept)
    assert (got[kept:].view(np.uint8) == 0xA5).all(), what


def _far_check(far, msg_cap, byte_cap, messages=()):
    w = far.w
    want_data, want_dpkts, want_msgs, n_msgs, n_bytes = dl.far_expected(w, (DATA, DPKT, MSG), msg_cap, byte_cap, fixed=far.fixed)
    data, dpkts, msgs, d_bytes, got_msgs, got_bytes = far.call(msg_cap, byte_cap)
    assert (got_msgs, got_bytes) == (n_msgs, n_bytes)
    _same(data, want_data, len(want_data), "connection")
    _same_records(dpkts, want_dpkts, "candidate")
    _same_records(msgs, want_msgs, "message")
    size = w.frags * dl.FAR_L
    stored = min(n_msgs, msg_cap, byte_cap // size)
    assert int((want_msgs["flags"] & dm.STORED != 0).sum()) == stored
    for M in messages:
        assert M < stored
        got = d_bytes[M * size:(M + 1) * size].cpu().numpy().tobytes()
        assert got == dl.far_octets(w, M), "the octets of message %d" % M
    assert bool((d_bytes[stored * size:] == 0xA5).all())                           # nothing behind the stored prefix
    return n_msgs, n_bytes


def test_the_far_world_at_a_small_size():
    """The device path the full size takes, where every octet can be compared."""
    far = _Far(dl.far_world((3, 40, 5, 2), 5, (CAND, CONN, PKT)))
    n_msgs, n_bytes = _far_check(far, 1 << 10, 1 << 20, messages=range(50))
    _far_check(far, 0, 0)
    _far_check(far, n_msgs, n_bytes, messages=(0, n_msgs - 1))
    _far_check(far, 17, 10 * 5 * 255 + 7, messages=(9,))


def test_the_far_world_beyond_2_to_32_octets():
    """100 + 65 600 + 150 + 50 messages of 65 535 octets: message 65 537 begins at 2^32 - 1, the second connection alone holds more
    than 2^32 octets, two connections lie behind the crossing, and the 32-bit running octet sums wrap."""
    t0 = time.time()
    far = _Far(dl.far_world(dl.FAR_COUNTS, dl.FAR_FRAGS, (CAND, CONN, PKT)))
    t1 = time.time()
    n_msgs, n_bytes = _far_check(far, 0, 0)
    assert n_bytes == 65900 * 65535 > 1 << 32 and far.n == 16936301
    t2 = time.time()
    _far_check(far, n_msgs, n_bytes, messages=(0, 65535, 65536, 65537, 65538, 65539, n_msgs - 1))
    t3 = time.time()
    print("far world: build and upload %.1f s, the call without room %.1f s, the call with room for everything %.1f s" % (t1 - t0, t2 - t1, t3 - t2))
