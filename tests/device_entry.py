"""Plumbing of tests/test_device_entry_gpu.py: what a device-resident caller of gnx_align_batch_device / gnx_score_batch_device supplies
itself -- input buffers and window tables in device memory, output buffers with a capacity, a stream -- laid out in torch tensors, with
guards behind every output.  Torch allocates, fills, copies and delays; nothing here computes a result.

Layout of an input (a Problem): one byte buffer per side and a (start, length) table per side, as the C ABI takes them.  concat() lays
lists of sequences out one behind the other (in input order or the other way round, so that the start tables descend); the tests build
the layouts with shared and overlapping windows themselves.  Every device input buffer is pre-filled with valid bases 0 .. 3 and has
64 spare bytes, so that a stale or misplaced read gives a wrong answer, never a bad base; the base pointer handed to the library may sit
1 .. 15 bytes into the allocation (a_shift / b_shift).

Outputs: d_ops is capacity + guard elements with guard >= T + 1024 (T: the oracle's run count), so that even a wholly unchecked write
of the full result stays inside the allocation; d_score and d_ops_off have 64 guard elements.  Every byte is 0xA5 before the call, and
Result.guards tells which guard changed.  The outputs are read with .cpu() on the default stream directly after the call, with no
synchronisation: "the call returns after the kernels finished" is part of what every test checks."""
import collections

import numpy as np
import torch

from gonomics_amd import _lib

FILL = 0xA5
TAIL_GUARD = 64     # guard elements behind d_score and d_ops_off
SPARE = 64          # bytes behind an input buffer

Problem = collections.namedtuple("Problem", "a_buf a_start a_len b_buf b_start b_len")
Result = collections.namedtuple("Result", "rc total scores ops off guards raw")  # (scores, ops, off): what common.assert_same takes


def _i64(x):
    return np.ascontiguousarray(x, dtype=np.int64)


def concat(alphas, betas, descending=False):
    """the sequences one behind the other; descending: the first pair's at the END of the buffers, so both start tables fall"""
    def side(seqs):
        lens = _i64([len(s) for s in seqs])
        order = range(len(seqs) - 1, -1, -1) if descending else range(len(seqs))
        start, at, parts = np.zeros(len(seqs), np.int64), 0, []
        for k in order:
            start[k] = at
            parts.append(np.asarray(seqs[k], np.uint8))
            at += len(seqs[k])
        buf = np.concatenate(parts) if at else np.zeros(0, np.uint8)
        return np.ascontiguousarray(buf, dtype=np.uint8), start, lens
    a, b = side(alphas), side(betas)
    return Problem(a[0], a[1], a[2], b[0], b[1], b[2])


def lists(pb):
    """(alphas, betas) of a Problem: what the oracle is given"""
    return ([pb.a_buf[s:s + l].copy() for s, l in zip(pb.a_start, pb.a_len)], [pb.b_buf[s:s + l].copy() for s, l in zip(pb.b_start, pb.b_len)])


def decoy_of(pb):
    """the same lengths on other data: both buffers reversed and every window at start 0 (in bounds whatever the lengths)"""
    return Problem(np.ascontiguousarray(pb.a_buf[::-1]), np.zeros_like(pb.a_start), pb.a_len, np.ascontiguousarray(pb.b_buf[::-1]), np.zeros_like(pb.b_start), pb.b_len)


class DeviceInputs:
    """a Problem in device memory (uploaded on torch's current stream)"""

    def __init__(self, pb, a_shift=0, b_shift=0):
        self.pb, self.n = pb, int(pb.a_start.shape[0])
        self.a_shift, self.b_shift = a_shift, b_shift
        self.a_all, self.a = self._buf(pb.a_buf, a_shift)
        self.b_all, self.b = self._buf(pb.b_buf, b_shift)
        self.a_start = torch.from_numpy(_i64(pb.a_start) if self.n else np.zeros(1, np.int64)).cuda()
        self.b_start = torch.from_numpy(_i64(pb.b_start) if self.n else np.zeros(1, np.int64)).cuda()

    @staticmethod
    def _buf(data, shift):
        whole = (torch.arange(data.shape[0] + shift + SPARE, device="cuda") % 4).to(torch.uint8)  # valid bases before, behind and (until the copy) under the data
        view = whole[shift:shift + data.shape[0]]
        if data.shape[0]:
            view.copy_(torch.from_numpy(data))
        assert shift == 0 or (whole.data_ptr() + shift) % 16 == shift % 16  # (torch's allocations are 16-byte aligned: the shift is the address's)
        return whole, view

    def overwrite_later(self, pb, stream, pinned):
        """queues, on `stream`, non-blocking copies of another Problem of the same lengths (from the pinned tensors of pin()) over this one"""
        with torch.cuda.stream(stream):
            self.a.copy_(pinned[0], non_blocking=True)
            self.b.copy_(pinned[1], non_blocking=True)
            self.a_start.copy_(pinned[2], non_blocking=True)
            self.b_start.copy_(pinned[3], non_blocking=True)
        self.pb = pb

    def poke(self, side, at, value):
        (self.a if side == "a" else self.b)[at] = value

    def args(self):
        return (self.a_all.data_ptr() + self.a_shift, self.a_start.data_ptr(), self.b_all.data_ptr() + self.b_shift, self.b_start.data_ptr(), _i64(self.pb.a_len), _i64(self.pb.b_len))


def pin(pb):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in (pb.a_buf, pb.b_buf, _i64(pb.a_start), _i64(pb.b_start)))


class Outputs:
    """d_score[n + 64], d_ops[capacity + guard], d_ops_off[n + 1 + 64], every byte 0xA5"""

    def __init__(self, n, capacity, T, after=None):
        self.n, self.capacity = n, int(capacity)
        self.guard = int(T) + 1024
        self.score = torch.full(((n + TAIL_GUARD) * 8,), FILL, dtype=torch.uint8, device="cuda")
        self.ops = torch.full(((self.capacity + self.guard) * 16,), FILL, dtype=torch.uint8, device="cuda")
        self.off = torch.full(((n + 1 + TAIL_GUARD) * 8,), FILL, dtype=torch.uint8, device="cuda")
        _ordered(after)

    def read(self):
        """the three buffers on the host, read on the default stream with no synchronisation before"""
        return self.score.cpu().numpy(), self.ops.cpu().numpy(), self.off.cpu().numpy()


def _ordered(stream):
    """what torch's current stream was given so far (the fill of the outputs) comes before what `stream` is given from now on"""
    if stream is not None and not isinstance(stream, int):
        stream.wait_stream(torch.cuda.current_stream())


def stream_handle(stream):
    """the hipStream_t of None (torch's current stream), 0 (the NULL stream) or a torch stream, as an integer"""
    if stream is None:
        return int(torch.cuda.current_stream().cuda_stream)
    return 0 if isinstance(stream, int) else int(stream.cuda_stream)


def _collect(n, out, rc, total, T_read):
    score_b, ops_b, off_b = out.read()
    guards = {"score": bool((score_b[n * 8:] == FILL).all()), "ops": bool((ops_b[out.capacity * 16:] == FILL).all()),
              "off": bool((off_b[(n + 1) * 8:] == FILL).all())}
    scores = score_b[:n * 8].view(np.int64).copy()
    off = off_b[:(n + 1) * 8].view(np.int64).copy()
    ops = np.frombuffer(ops_b[:max(0, min(T_read, out.capacity)) * 16].tobytes(), dtype=_lib.CIGAR_DTYPE).copy()
    return Result(rc, total, scores, ops, off, guards, (score_b, ops_b, off_b))


def align(params, dev, capacity, T, stream=None, want_total=True, n_pairs=None, prepared=False, guard_T=None):
    """one gnx_align_batch_device call on a DeviceInputs with fresh, guarded outputs; T: the oracle's run count (sizes the guard and tells
    how many runs to hand back).  Inputs uploaded on torch's current stream are finished first unless the caller ordered them itself
    (prepared: they were queued on the very stream the call gets)."""
    n = dev.n if n_pairs is None else n_pairs
    out = Outputs(n, capacity, T if guard_T is None else guard_T, after=stream if prepared else None)
    if not prepared:
        torch.cuda.synchronize()
    a, a_s, b, b_s, al, bl = dev.args()
    rc, total = _lib.align_batch_device(params, n, a, a_s, b, b_s, al, bl, out.score.data_ptr(), out.ops.data_ptr(), capacity, out.off.data_ptr(),
                                        stream=stream_handle(stream), want_total=want_total)
    return _collect(n, out, rc, total, T)


def score(params, dev, stream=None, prepared=False, n_pairs=None):
    """one gnx_score_batch_device call: (rc, scores, the d_score guard's state)"""
    n = dev.n if n_pairs is None else n_pairs
    d_score = torch.full(((n + TAIL_GUARD) * 8,), FILL, dtype=torch.uint8, device="cuda")
    if prepared:
        _ordered(stream)
    else:
        torch.cuda.synchronize()
    a, a_s, b, b_s, al, bl = dev.args()
    rc = _lib.score_batch_device(params, n, a, a_s, b, b_s, al, bl, d_score.data_ptr(), stream=stream_handle(stream))
    sb = d_score.cpu().numpy()
    return rc, sb[:n * 8].view(np.int64).copy(), bool((sb[n * 8:] == FILL).all())


# ---- the delay of the stream tests ---------------------------------------------------------------------------------------------------------
_DELAY = {}


def _spin(stream, amount):
    with torch.cuda.stream(stream):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(amount))
        else:  # a chain of dependent large operations
            x = _DELAY.setdefault("x", torch.ones(1 << 24, device="cuda"))
            for _ in range(int(amount)):
                x.mul_(1.0000001)


def delay(stream, want_ms=40.0):
    """queues a delay of about want_ms on `stream` between two events and returns them: its length is MEASURED, once for the rate (here)
    and by the caller for the delay it actually got (elapsed_time of the two events, after the call under test has returned)"""
    if "rate" not in _DELAY:
        unit = 2000000 if hasattr(torch.cuda, "_sleep") else 8
        _spin(stream, unit)  # (warm-up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        _spin(stream, unit)
        e1.record(stream)
        e1.synchronize()
        _DELAY["rate"] = unit / max(e0.elapsed_time(e1), 1e-3)  # units per millisecond
        _DELAY["unit"] = unit
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    _spin(stream, min(max(1, int(_DELAY["rate"] * want_ms)), 100 * _DELAY["unit"]))  # (bounded whatever was measured; the caller asserts what it got)
    e1.record(stream)
    return e0, e1
