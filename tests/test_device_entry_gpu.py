"""The device-resident entries, gnx_align_batch_device and gnx_score_batch_device, called as a device-resident caller calls them.

Every other GPU suite reaches run_device and score_or_fallback through the host flows, which supply their own stream, grow their own
CIGAR buffer, upload into aligned buffers and rebase the window tables.  A caller of the device entries supplies all of that itself,
and bench.py's headline is timed through gnx_align_batch_device.  Here (tests/device_entry.py does the plumbing):

A  every align route of the catalogue of tests/test_scratch_state_gpu.py (ROUTES / ALIGN_KEYS / ROUTE_SWITCHES: it exists once, there,
   and nothing else of that module is used), the forced
   gapless certificate and a mixed batch, one call each on torch's current stream with capacity T + 7;
B  layouts no host flow produces: base pointers 1, 7 and 15 bytes into an allocation, descending window tables, windows of one shared
   chunk that overlap, alpha windows that overlap or are named by several pairs, no pairs at all, out_total_ops == NULL; the
   pointer offsets and the descending tables also on a batch whose reads ARE certified (fp1's never are, see below);
C  streams: the NULL stream, a stream of the caller's on which the inputs arrive late, outputs read with no synchronisation, two
   streams in turn;
D  the capacity contract: capacities T, T - 1, T / 2, 1 and 0 -- the need reported with GNX_ECAPACITY is the whole batch's, nothing
   is written at or behind element `capacity`, and the call after a refusal is the oracle's;
E  errors and the call after them;  F  device-entry calls between host-flow calls on one context;  G  gnx_score_batch_device.

Expected values are the oracle's (asym.expected for the batches of tests/asym.py, oracle.align_batch otherwise), never a host entry's;
every comparison is exact.  Guards: 0xA5 behind every output, checked after every call.

Two places where the batches differ from what one would first write down, both decided by the inputs alone:
* the mixed batch.  Under GNX_FASTPATH=2 the fast path takes every pair with 1 .. 20 480 rows, so no pair of tests/asym.py's batches has
  key 0 there and the general-path group of the mixed block would not run.  MIXED is therefore 256 pairs (fp1, fp2, fp3 and small
  interleaved pair by pair, each batch repeated from its start) under the library's own rule, where windows of fewer than 768 columns
  are key 0: four keys, 0 among them (asserted from the lengths).  The 64-pair batch under GNX_FASTPATH=2 (keys 1, 2, 3) runs as well.
* the forced certificate on fp1.  No read of fp1 is gapless against its window (6 % substitutions), so the host's certificate admits
  none and counter 9 stays 0 whatever the kernel does; what is asserted there is counter 10 == 56 and counters 9 + 11 == the host's count.
  The catalogue's own certificate batch (18 of 24 certified) runs through the device entry too, with both counters non-zero."""
import collections
import functools

import numpy as np
import pytest
import torch

import asym
import common
import device_entry as de
import oracle
import test_scratch_state_gpu as cat
from asym import ASYM
from gonomics_amd import _lib

pytestmark = pytest.mark.gpu

Subject = collections.namedtuple("Subject", "what env pb exp mode mx go ge ci route")
OK, ECAP = _lib.GNX_OK, _lib.GNX_ECAPACITY
GO, GE = -600, -150


@pytest.fixture(autouse=True)
def _own_switches(monkeypatch):
    for k in cat.ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")


def _params(s):
    return _lib.make_params(s.mode, s.mx, s.go, s.ge, s.ci, s.ci)


def _T(s):
    return int(s.exp[2][-1])


# ---- subjects: a batch, its layout, the oracle's result, the switches of its route -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def named(name, mode, go, ge, ci, route, env, descending=False):
    """a batch of tests/asym.py, its sequences one behind the other"""
    alphas, betas = asym.batch(name)
    return Subject("%s mode %d (%d, %d) checkersize %d%s" % (name, mode, go, ge, ci, " descending" if descending else ""), dict(env), de.concat(alphas, betas, descending),
                   asym.expected(name, mode, "ASYM", go, ge, ci), mode, ASYM, go, ge, ci, route)


def of_key(key):
    name, mode, go, ge, ci, route = cat.ROUTES[key].align
    return named(name, mode, go, ge, ci, route, tuple(sorted(cat.ROUTES[key].env.items())))


def _env(**kw):
    return tuple(sorted(kw.items()))


B_ROUTES = collections.OrderedDict([("fast_path_cert", ("fp1", 1, _env(GNX_FASTPATH="2", GNX_FP_CERT="2"))), ("stored", ("small", 0, _env(GNX_FASTPATH="0"))),
                                    ("snapshot16", ("long40", 2, _env(GNX_CLONG="2", GNX_W64="0")))])


def of_route(r, descending=False):
    name, route, env = B_ROUTES[r]
    return named(name, 0, GO, GE, 10000, route, env, descending)


def key_of(n, m, forced, n_pairs):
    """run_device's key of a pair (rows n, columns m; global affine, not transposed): its number of 160-row blocks, 0 = not for the fast path"""
    assert (n + m + 2) * 600 < (1 << 27)
    if n < 1 or m < 1:
        return 0
    blocks = (n + 159) // 160
    if blocks > 128 or (not forced and m < (32 if n_pairs >= 8192 else 768)):
        return 0
    return blocks


@functools.lru_cache(maxsize=None)
def mixed(forced=False):
    parts = [asym.batch(b) for b in ("fp1", "fp2", "fp3", "small")]
    alphas, betas = [], []
    for k in range(16 if forced else 64):
        for a, b in parts:
            alphas.append(a[k % len(a)]); betas.append(b[k % len(b)])
    keys = {key_of(len(a), len(b), forced, len(alphas)) for a, b in zip(alphas, betas)}
    assert len(keys) >= 3 and (forced or 0 in keys), keys  # the block of run_device for batches with more than one key runs, with a general-path group
    assert forced or len(alphas) >= 256                   # (fewer pairs with several keys stay off the fast path altogether)
    env = _env(GNX_FASTPATH="2") if forced else _env(GNX_LAT="0")
    return Subject("mixed batch%s" % (" forced" if forced else ""), dict(env), de.concat(alphas, betas), oracle.align_batch(0, ASYM, GO, GE, alphas, betas, threads=8),
                   0, ASYM, GO, GE, 10000, 1)


@functools.lru_cache(maxsize=None)
def shared_chunk(r, alpha_mode):
    """bench.py's shape scaled down: one chunk of 3 000 bases, 96 reads of 1 .. 160 bases, every window a slice of the chunk of 200 .. 700
    columns at an arbitrary start (they overlap), all pairs on one beta buffer.  alpha_mode: own = every read its own bytes; dup = 48
    reads, each named by two pairs; overlap = the reads are overlapping slices of ONE mutated copy of the chunk"""
    rng = np.random.default_rng(7200)
    chunk = rng.integers(0, 4, size=3000).astype(np.uint8)
    chunk[rng.integers(0, 3000, size=6)] = 4
    n = 96
    a_len = np.asarray([1, 2, 159, 160] + [int(x) for x in rng.integers(1, 161, size=n - 4)], np.int64)
    b_len = rng.integers(200, 701, size=n).astype(np.int64)
    b_start = np.asarray([int(rng.integers(0, 3000 - m + 1)) for m in b_len], np.int64)
    pos = np.asarray([int(rng.integers(0, m - a + 1)) for a, m in zip(a_len, b_len)], np.int64)
    if alpha_mode == "overlap":
        a_buf = common.mutate(rng, chunk, 0.05, 0.01)
        a_start = np.minimum(b_start + pos, a_buf.shape[0] - a_len)
    else:
        reads = []
        for k in range(n if alpha_mode == "own" else n // 2):
            w = chunk[b_start[k] + pos[k]:b_start[k] + pos[k] + a_len[k] + 20]
            x = common.mutate(rng, w, 0.06, 0.02)[:a_len[k]]
            reads.append(np.concatenate([x, rng.integers(0, 4, size=a_len[k] - x.shape[0]).astype(np.uint8)]))
        a_buf = np.concatenate(reads)
        starts = np.concatenate([[0], np.cumsum([len(x) for x in reads])[:-1]]).astype(np.int64)
        if alpha_mode == "dup":
            a_len = np.concatenate([a_len[:n // 2], a_len[:n // 2]])
            a_start = np.concatenate([starts, starts])
        else:
            a_start = starts
    pb = de.Problem(np.ascontiguousarray(a_buf, dtype=np.uint8), a_start.astype(np.int64), a_len, chunk, b_start, b_len)
    if alpha_mode == "dup":
        assert len(set(a_start.tolist())) == n // 2
    if alpha_mode == "overlap":
        order = np.argsort(a_start)
        assert (a_start[order][1:] < (a_start + a_len)[order][:-1]).any()
    order = np.argsort(b_start)
    assert (b_start[order][1:] < (b_start + b_len)[order][:-1]).sum() > n // 2  # the windows overlap
    alphas, betas = de.lists(pb)
    name, route, env = B_ROUTES[r]
    return Subject("shared chunk, alpha %s, %s" % (alpha_mode, r), dict(env), pb, oracle.align_batch(0, ASYM, GO, GE, alphas, betas, threads=8), 0, ASYM, GO, GE, 10000, route)


def _per_subject(fn):
    """computed once per subject (its `what` names its data: subjects that differ in their switches alone share it)"""
    memo = {}

    def wrapped(s, *args):
        if (s.what,) + args not in memo:
            memo[(s.what,) + args] = fn(s, *args)
        return memo[(s.what,) + args]
    return wrapped


@_per_subject
def reversed_twin(s):
    """the same lengths, every sequence reverse-complemented (a read stays related to its window; under ASYM the scores are others, which
    those of merely reversed sequences would not be): the other batch of the two-stream test"""
    alphas, betas = de.lists(s.pb)
    alphas, betas = [asym.rc(a) for a in alphas], [asym.rc(b) for b in betas]
    return s._replace(what=s.what + " reverse-complemented", pb=de.concat(alphas, betas), exp=oracle.align_batch(s.mode, s.mx, s.go, s.ge, alphas, betas, s.ci, s.ci, threads=8))


@_per_subject
def decoy_expected(s):
    alphas, betas = de.lists(de.decoy_of(s.pb))
    return oracle.align_batch(s.mode, s.mx, s.go, s.ge, alphas, betas, s.ci, s.ci, threads=8)


@_per_subject
def device(s, a_shift=0, b_shift=0):
    """the subject's inputs in device memory, uploaded once (tests that change them build their own)"""
    return de.DeviceInputs(s.pb, a_shift, b_shift)


def stream_subject(which):
    return mixed() if which == "mixed" else of_route(which)


# ---- what every call is held against ---------------------------------------------------------------------------------------------------------
def apply(monkeypatch, s):
    for k, v in s.env.items():
        monkeypatch.setenv(k, v)


def accepted(res, s, what="", total=True):
    what = "%s %s" % (s.what, what)
    assert res.rc == OK, (what, res.rc, _lib.last_error())
    if total:
        assert res.total == _T(s), (what, res.total, _T(s))
    assert res.off.shape[0] == s.pb.a_start.shape[0] + 1
    common.assert_same((res.scores, res.ops, res.off), s.exp, what)
    assert all(res.guards.values()), (what, res.guards)


def refused(res, s, what=""):
    what = "%s %s" % (s.what, what)
    assert res.rc == ECAP, (what, res.rc)
    assert res.total == _T(s), (what, "the need reported is not the whole batch's", res.total, _T(s))
    assert all(res.guards.values()), (what, res.guards)


def routed(s, what=""):
    """the route assertion of the scratch-state suite: the families 0 / 1 / 2 through common.expect_route, the others exactly -- and none
    at all under a route switch set outside the suite (tools/switch_matrix.sh), where only the equality stays"""
    tm = _lib.get_timing()
    if s.route in (0, 1, 2):
        common.expect_route(tm, s.route)
    elif s.route is not None and not common.OUTER_ROUTE_SWITCH:
        assert tm["fast_path"] == s.route, (tm["fast_path"], s.route, s.what, what)


def one_call(monkeypatch, s, dev=None, **kw):
    apply(monkeypatch, s)
    res = de.align(_params(s), dev or device(s), kw.pop("capacity", _T(s) + 7), _T(s), **kw)
    return res


# ---- A: every route through the device entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", cat.ALIGN_KEYS)
def test_every_route(gpu_lib, monkeypatch, key):
    s = of_key(key)
    accepted(one_call(monkeypatch, s), s, key)
    routed(s, key)


def test_every_align_key_is_a_case():
    assert len(cat.ALIGN_KEYS) >= 100 and all(cat.ROUTES[k].align for k in cat.ALIGN_KEYS)


def _counters():
    return _lib.debug_counter(9), _lib.debug_counter(10), _lib.debug_counter(11)


def test_forced_certificate_fp1(gpu_lib, monkeypatch):
    s = named("fp1", 0, GO, GE, 10000, 1, _env(GNX_FASTPATH="2", GNX_FP_CERT="2"))
    alphas, betas = asym.batch("fp1")
    host = sum(1 for a, b in zip(alphas, betas) if _lib.debug_gapless_certificate_n(_params(s), a, b, K=16)[0])
    _counters()
    accepted(one_call(monkeypatch, s), s)
    routed(s)
    c9, c10, c11 = _counters()
    print("fp1: certified %d + %d of %d offered, host %d" % (c9, c11, c10, host))
    assert host == 0  # no read of fp1 is gapless against its window: were that to change, counter 9 > 0 is what belongs here
    assert c10 == len(alphas) > 0 and c9 + c11 == host


@functools.lru_cache(maxsize=None)
def certificate_subject(descending=False):
    """the batch of the catalogue's case fast_path/certificate_forced (tests/test_fp_cert_gpu.py's generator with that case's arguments:
    18 pairs whose certificate the construction decides, 6 with an indel), and how many of its pairs the host's certificate admits"""
    import test_fp_cert_gpu as tfc
    reads, wins, exp, meta = tfc.batch(4124, 24, kinds=tfc.SURE + ("indel",), ms=(300, 2000), ns=tfc.N_CERTIFIABLE)
    s = Subject("the catalogue's certificate batch%s" % (" descending" if descending else ""), dict(GNX_FASTPATH="2", GNX_FP_CERT="2"),
                de.concat(list(reads), list(wins), descending), exp, 0, tfc.HCT, tfc.GO, tfc.GE, 10000, 1)
    host = sum(1 for a, b in zip(reads, wins) if _lib.debug_gapless_certificate(_params(s), a, b, K=16)[0])
    assert 0 < host < len(reads)
    return s, host


def certified_call(monkeypatch, s, host, dev=None, what=""):
    """one call of the certificate batch: the oracle's result, and the kernel certified exactly the pairs the host's certificate admits"""
    _counters()
    accepted(one_call(monkeypatch, s, dev=dev), s, what)
    routed(s)
    c9, c10, c11 = _counters()
    assert c9 > 0 and c10 > 0 and (c9 + c11, c10) == (host, s.pb.a_start.shape[0]), (what, c9, c10, c11, host)


def test_forced_certificate_catalogue_batch(gpu_lib, monkeypatch):
    s, host = certificate_subject()
    certified_call(monkeypatch, s, host)


@pytest.mark.parametrize("forced", [False, True], ids=["own_rule_256", "forced_64"])
def test_mixed_batch(gpu_lib, monkeypatch, forced):
    s = mixed(forced)
    accepted(one_call(monkeypatch, s), s)
    routed(s)


# ---- B: layouts the host flows never produce -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [(1, 7), (7, 15), (15, 1)], ids=lambda x: "alpha+%d_beta+%d" % x)
@pytest.mark.parametrize("r", list(B_ROUTES))
def test_base_pointers_inside_an_allocation(gpu_lib, monkeypatch, r, shifts):
    s = of_route(r)
    accepted(one_call(monkeypatch, s, dev=device(s, *shifts)), s, shifts)
    routed(s)


@pytest.mark.parametrize("shifts", [(1, 7), (7, 15), (15, 1), (0, 1), (0, 15)], ids=lambda x: "alpha+%d_beta+%d" % x)
def test_certified_reads_at_unaligned_addresses(gpu_lib, monkeypatch, shifts):
    """fp1 has no gapless read, so on it the certificate only ever refuses; here 18 of 24 reads are certified and leave through the
    certificate's own output path, with fp_cert_kernel's 16-byte grid taken from a window address that is 1, 7 or 15 bytes off"""
    s, host = certificate_subject()
    certified_call(monkeypatch, s, host, dev=device(s, *shifts), what=str(shifts))


def test_certified_reads_descending_tables(gpu_lib, monkeypatch):
    s, host = certificate_subject(descending=True)
    assert (np.diff(s.pb.b_start) < 0).all()
    certified_call(monkeypatch, s, host)


@pytest.mark.parametrize("r", list(B_ROUTES))
def test_descending_window_tables(gpu_lib, monkeypatch, r):
    s = of_route(r, descending=True)
    assert (np.diff(s.pb.a_start) <= 0).all() and (np.diff(s.pb.b_start) <= 0).all() and s.pb.a_start[0] > 0
    accepted(one_call(monkeypatch, s), s)
    routed(s)


@pytest.mark.parametrize("alpha_mode", ["own", "dup", "overlap"])
@pytest.mark.parametrize("r", list(B_ROUTES))
def test_windows_of_one_shared_chunk(gpu_lib, monkeypatch, r, alpha_mode):
    s = shared_chunk(r, alpha_mode)
    accepted(one_call(monkeypatch, s), s)
    routed(s)


@pytest.mark.parametrize("r", list(B_ROUTES))
def test_no_pairs(gpu_lib, monkeypatch, r):
    """GNX_OK, d_ops_off[0] == 0, total 0, and not one other byte of the outputs written"""
    s = of_route(r)
    apply(monkeypatch, s)
    res = de.align(_params(s), device(s), 16, 0, n_pairs=0)
    assert (res.rc, res.total) == (OK, 0) and res.off.tolist() == [0]
    score_b, ops_b, off_b = res.raw
    assert (score_b == de.FILL).all() and (ops_b == de.FILL).all() and (off_b[8:] == de.FILL).all()


@pytest.mark.parametrize("r", list(B_ROUTES))
def test_no_total_pointer(gpu_lib, monkeypatch, r):
    s = of_route(r)
    res = one_call(monkeypatch, s, want_total=False)
    assert res.total is None
    accepted(res, s, "out_total_ops == NULL", total=False)
    routed(s)


# ---- C: streams ------------------------------------------------------------------------------------------------------------------------------
STREAM_SUBJECTS = list(B_ROUTES) + ["mixed"]


@pytest.mark.parametrize("which", STREAM_SUBJECTS)
def test_null_stream(gpu_lib, monkeypatch, which):
    s = stream_subject(which)
    accepted(one_call(monkeypatch, s, stream=0), s, "NULL stream")
    routed(s)


@pytest.mark.parametrize("which", STREAM_SUBJECTS)
def test_inputs_arrive_late_on_the_callers_stream(gpu_lib, monkeypatch, which):
    """On a stream of the caller's: a delay (tens of milliseconds, measured), then the real inputs copied from pinned memory over decoy
    inputs of the same lengths, then the call with that stream.  "Same stream" is all that orders the call behind the copies: a library
    that ran anything that reads the inputs elsewhere would align the decoy, whose scores are not the real ones'.  The outputs are read
    on the default stream with no synchronisation: the call returns after its kernels finished."""
    s = stream_subject(which)
    decoy = decoy_expected(s)
    assert not np.array_equal(decoy[0], s.exp[0]) and np.mean(decoy[0] != s.exp[0]) > 0.5
    apply(monkeypatch, s)
    accepted(de.align(_params(s), device(s), _T(s) + 7, _T(s)), s, "warm-up")  # the workspace has its size: no allocation (a device-wide wait) in the call under test
    pinned = de.pin(s.pb)
    # twice, on two streams created one after the other: streams share the few hardware queues, and work that a library put on a stream
    # of its own would queue behind the delay all the same if that stream and the caller's fell on one queue -- two neighbours do not both
    for st in (torch.cuda.Stream(), torch.cuda.Stream()):
        dev = de.DeviceInputs(de.decoy_of(s.pb))
        torch.cuda.synchronize()  # the decoy is in place
        e0, e1 = de.delay(st)
        dev.overwrite_later(s.pb, st, pinned)
        res = de.align(_params(s), dev, _T(s) + 7, _T(s), stream=st, prepared=True, guard_T=max(_T(s), int(decoy[2][-1])))
        ms = e0.elapsed_time(e1)
        print("delay in front of the inputs: %.1f ms" % ms)
        assert ms >= 20.0, ms  # (the delay really was long against the host's way from the copies to the call)
        assert not np.array_equal(res.scores, decoy[0]), "the decoy was aligned: something read the inputs off the caller's stream"
        accepted(res, s, "inputs late on a fresh stream")
        routed(s)


@pytest.mark.parametrize("which", STREAM_SUBJECTS)
def test_outputs_are_final_on_return(gpu_lib, monkeypatch, which):
    """a fresh stream, the outputs read with .cpu() on the default stream directly after the return (de.align does no more than that)"""
    s = stream_subject(which)
    st = torch.cuda.Stream()
    assert st.cuda_stream != torch.cuda.current_stream().cuda_stream
    accepted(one_call(monkeypatch, s, stream=st), s, "fresh stream")
    routed(s)


@pytest.mark.parametrize("which", STREAM_SUBJECTS)
def test_two_streams_in_turn(gpu_lib, monkeypatch, which):
    """two calls in a row on two streams with two batches: the workspace is one, and each result is its own batch's"""
    s = stream_subject(which)
    t = reversed_twin(s)
    assert np.mean(s.exp[0] != t.exp[0]) > 0.5
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    apply(monkeypatch, s)
    first = de.align(_params(s), device(s), _T(s) + 7, _T(s), stream=s1)
    second = de.align(_params(t), device(t), _T(t) + 7, _T(t), stream=s2)
    third = de.align(_params(s), device(s), _T(s) + 7, _T(s), stream=s2)
    accepted(first, s, "first, stream 1")
    accepted(second, t, "second, stream 2")
    accepted(third, s, "third, stream 2")


# ---- D: the capacity contract ----------------------------------------------------------------------------------------------------------------
def _with(s, **more):
    return s._replace(env=dict(s.env, **more))


FAMILIES = collections.OrderedDict([
    ("stored_hform", lambda: of_key("stored_hform/small/mode0")),
    ("stored_workspace_chunks", lambda: named("long40", 0, GO, GE, 10000, 0, _env(GNX_FASTPATH="0", GNX_CLONG="0"))),
    ("latency", lambda: of_key("latency/tall12/mode0")),
    ("int64", lambda: of_key("int64/long16/mode0")),
    ("fast_path_1_block_cert_off", lambda: _with(of_key("fast_path/1_blocks/global"), GNX_FP_CERT="0")),
    ("fast_path_1_block_cert_on", lambda: _with(of_key("fast_path/1_blocks/global"), GNX_FP_CERT="2")),
    ("fast_path_3_blocks", lambda: of_key("fast_path/3_blocks/global")),
    ("fast_path_transposed", lambda: of_key("fast_path/2_blocks/transposed")),
    ("fast_path_overflow_redo", lambda: of_key("fast_path/overflow_redo/global")),
    ("mixed", lambda: mixed()),
    ("mixed_forced", lambda: mixed(True)),
    ("snapshot16", lambda: of_key("snapshot16/static/mode0/checker10000")),
    ("snapshot64_farm", lambda: of_key("snapshot64/farm/mode0/checker10000")),
    ("row_panels16", lambda: of_key("row_panels16/mode0")),
    ("row_panels64", lambda: of_key("row_panels64/mode0"))])
CAPACITIES = collections.OrderedDict([("T", lambda T: T), ("T-1", lambda T: T - 1), ("half", lambda T: T // 2), ("1", lambda T: 1), ("0", lambda T: 0)])


@pytest.mark.parametrize("cap", list(CAPACITIES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_capacity_contract(gpu_lib, monkeypatch, family, cap):
    s = FAMILIES[family]()
    T = _T(s)
    capacity = CAPACITIES[cap](T)
    assert T > 2 and 0 <= capacity <= T
    apply(monkeypatch, s)
    small_ws = family == "stored_workspace_chunks"
    if small_ws:
        _lib.check(_lib.lib().gnx_init(0, 4 << 20))
    try:
        res = de.align(_params(s), device(s), capacity, T)
        print("%s capacity %d of %d: rc %d, total %r, guards %r" % (family, capacity, T, res.rc, res.total, res.guards))
        if capacity >= T:
            accepted(res, s, "capacity T")
            routed(s)
            if small_ws:
                assert _lib.get_timing()["n_launches"] > 1
        else:
            refused(res, s, "capacity %d" % capacity)
            again = de.align(_params(s), device(s), res.total, T)  # sized from the refusal, as bench.py sizes its buffer
            accepted(again, s, "after the refusal at capacity %d" % capacity)
            routed(s)
    finally:
        if small_ws:
            _lib.check(_lib.lib().gnx_init(0, 8 << 30))


# ---- E: errors and the call after them -------------------------------------------------------------------------------------------------------
E_ROUTES = collections.OrderedDict([("fast_path_cert_on", ("fp1", 1, _env(GNX_FASTPATH="2", GNX_FP_CERT="2"))), ("fast_path_cert_off", ("fp1", 1, _env(GNX_FASTPATH="2", GNX_FP_CERT="0"))),
                                    ("stored", B_ROUTES["stored"]), ("snapshot16", B_ROUTES["snapshot16"])])


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("pair", ["first", "middle", "last"])
@pytest.mark.parametrize("r", list(E_ROUTES))
def test_bad_base_then_clean(gpu_lib, monkeypatch, r, pair, side):
    name, route, env = E_ROUTES[r]
    s = named(name, 0, GO, GE, 10000, route, env)
    n = s.pb.a_start.shape[0]
    k = {"first": 0, "middle": n // 2, "last": n - 1}[pair]
    start, length = (s.pb.a_start[k], s.pb.a_len[k]) if side == "a" else (s.pb.b_start[k], s.pb.b_len[k])
    at = int(start + length // 2)
    apply(monkeypatch, s)
    dev = de.DeviceInputs(s.pb)
    dev.poke(side, at, 9)
    res = de.align(_params(s), dev, _T(s) + 7, _T(s))
    assert res.rc == _lib.GNX_EBASE, (res.rc, _lib.last_error())
    assert all(res.guards.values()), res.guards
    dev.poke(side, at, int((s.pb.a_buf if side == "a" else s.pb.b_buf)[at]))
    accepted(de.align(_params(s), dev, _T(s) + 7, _T(s)), s, "after GNX_EBASE")
    routed(s)


@pytest.mark.parametrize("mode", [0, 1])
def test_empty_sequence_in_a_low_memory_mode(gpu_lib, mode):
    alphas, betas = asym.batch("small")
    alphas, betas = list(alphas[:8]), list(betas[:8])
    alphas[5] = np.zeros(0, np.uint8)
    dev = de.DeviceInputs(de.concat(alphas, betas))
    go, ge = asym.pens(mode)[-1]
    res = de.align(_lib.make_params(mode, ASYM, go, ge), dev, 64, 64)
    assert res.rc == _lib.GNX_EEMPTY and all(res.guards.values())


def test_invalid_arguments(gpu_lib):
    s = of_route("stored")
    dev, p = device(s), _params(s)
    a, a_s, b, b_s, al, bl = dev.args()
    out = de.Outputs(dev.n, _T(s) + 7, _T(s))
    torch.cuda.synchronize()
    sc, ops, off, cap = out.score.data_ptr(), out.ops.data_ptr(), out.off.data_ptr(), _T(s) + 7
    call = _lib.align_batch_device
    assert call(p, dev.n, a, a_s, b, b_s, al, bl, 0, ops, cap, off)[0] == _lib.GNX_EINVAL
    assert call(p, dev.n, a, a_s, b, b_s, al, bl, sc, ops, cap, 0)[0] == _lib.GNX_EINVAL
    assert call(p, dev.n, a, a_s, b, b_s, al, bl, sc, ops, -1, off)[0] == _lib.GNX_EINVAL
    assert call(p, dev.n, a, a_s, b, b_s, None, bl, sc, ops, cap, off)[0] == _lib.GNX_EINVAL
    assert _lib.score_batch_device(p, dev.n, a, a_s, b, b_s, al, bl, 0) == _lib.GNX_EINVAL
    assert _lib.score_batch_device(p, dev.n, a, a_s, b, b_s, None, bl, sc) == _lib.GNX_EINVAL
    assert all((x == de.FILL).all() for x in out.read())  # a refused call writes nothing
    rc, total = call(p, dev.n, a, a_s, b, b_s, al, bl, sc, ops, cap, off)
    assert (rc, total) == (OK, _T(s))


# ---- F: device-entry calls between host-flow calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dirty", [False, True], ids=["as_left", "scratch_filled"])
def test_history_between_host_flows(gpu_lib, dirty):
    """a packed-beta host call, the device entry on byte windows, the packed-beta call again, the device score entry, a plain host call:
    the context's packed-beta flag and its cached plans are set and restored around the host flows, and the device entries read neither"""
    L = gpu_lib
    ref, reads, w_start, w_len = asym.global_ref_batch()
    cat_reads = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    exp = oracle.align_batch(0, ASYM, GO, GE, reads, [ref[b:b + l] for b, l in zip(w_start, w_len)], threads=8)
    p = L.make_params(0, ASYM, GO, GE)
    s = Subject("reads against windows of the reference as bytes", {}, de.Problem(cat_reads, off[:-1].copy(), np.diff(off), ref, w_start, w_len), exp, 0, ASYM, GO, GE, 10000, None)
    dev = de.DeviceInputs(s.pb)

    def between():
        if dirty:
            assert L.debug_fill_scratch(0x80808080)[0] > 0
    L.set_reference(ref)
    try:
        common.assert_same(L.align_batch_by_offset(p, cat_reads, off, w_start, w_len), exp, "step 1, by offset")
        between()
        accepted(de.align(p, dev, _T(s) + 7, _T(s)), s, "step 2, device entry")
        between()
        common.assert_same(L.align_batch_by_offset(p, cat_reads, off, w_start, w_len), exp, "step 3, by offset")
        between()
        rc, scores, guard = de.score(p, dev)
        assert rc == OK and guard and np.array_equal(scores, exp[0]), "step 4, device score entry"
        between()
        common.assert_same(L.align_batch(p, *asym.batch("small")), asym.expected("small", 0, "ASYM", GO, GE), "step 5, align_batch")
    finally:
        L.set_reference(np.zeros(0, np.uint8))


# ---- G: gnx_score_batch_device ---------------------------------------------------------------------------------------------------------------
def _score_subject(name, mode, go=None, ge=None):
    if go is None:
        go, ge = asym.pens(mode)[-1]
    return named(name, mode, go, ge, 10000, 8 if mode == 3 else 7, ())


def _score_route_is(route, what):
    if not common.OUTER_ROUTE_SWITCH:
        assert _lib.get_timing()["fast_path"] == route, (what, _lib.get_timing()["fast_path"], route)


SCORE_CASES = [(name, mode) for mode in range(5) for name in (("local" if mode == 3 else "sweep"), "small")]


@pytest.mark.parametrize("stream", ["current", "null", "fresh"])
@pytest.mark.parametrize("name,mode", SCORE_CASES)
def test_score_entry(gpu_lib, name, mode, stream):
    s = _score_subject(name, mode)
    st = {"current": None, "null": 0, "fresh": torch.cuda.Stream()}[stream]
    rc, scores, guard = de.score(_params(s), device(s), stream=st)
    assert rc == OK, (rc, _lib.last_error())
    _score_route_is(s.route, s.what)
    assert np.array_equal(scores, s.exp[0]), (s.what, np.flatnonzero(scores != s.exp[0])[:8])
    assert guard
    if stream == "current":  # the align entry on the same tensors
        res = de.align(_params(s), device(s), _T(s), _T(s))
        assert res.rc == OK and np.array_equal(res.scores, scores)


@pytest.mark.parametrize("which", STREAM_SUBJECTS[:3])
def test_score_entry_inputs_arrive_late(gpu_lib, monkeypatch, which):
    s = of_route(which)  # (the route switches are the align entry's: the score sweep takes all three batches)
    decoy = decoy_expected(s)
    assert de.score(_params(s), device(s))[0] == OK  # (warm-up, as above)
    pinned = de.pin(s.pb)
    for st in (torch.cuda.Stream(), torch.cuda.Stream()):  # (two neighbours, as above)
        dev = de.DeviceInputs(de.decoy_of(s.pb))
        torch.cuda.synchronize()
        e0, e1 = de.delay(st)
        dev.overwrite_later(s.pb, st, pinned)
        rc, scores, guard = de.score(_params(s), dev, stream=st, prepared=True)
        ms = e0.elapsed_time(e1)
        assert ms >= 20.0, ms
        assert rc == OK and guard and not np.array_equal(scores, decoy[0])
        assert np.array_equal(scores, s.exp[0])
        _score_route_is(7, s.what)


@pytest.mark.parametrize("which", STREAM_SUBJECTS)
def test_score_entry_two_streams_in_turn(gpu_lib, which):
    """two score calls in a row on two streams with two batches, then the first batch on the second stream: the sweep's workspace is
    one, and each result is its own batch's"""
    s = stream_subject(which)
    t = reversed_twin(s)
    assert np.mean(s.exp[0] != t.exp[0]) > 0.5
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for u, st, what in ((s, s1, "first, stream 1"), (t, s2, "second, stream 2"), (s, s2, "third, stream 2")):
        rc, scores, guard = de.score(_params(u), device(u), stream=st)
        assert rc == OK and guard, (what, rc, _lib.last_error())
        _score_route_is(7, (u.what, what))
        assert np.array_equal(scores, u.exp[0]), (u.what, what, np.flatnonzero(scores != u.exp[0])[:8])


@functools.lru_cache(maxsize=None)
def _fallback_subject(which):
    alphas, betas = asym.batch("small")
    if which == "gap_open_positive":
        mode, go, ge, env = 0, 25, GE, {}
    elif which == "sweep_switched_off":
        mode, go, ge, env = 0, GO, GE, {"GNX_SCORE_SWEEP": "0"}
    else:
        mode, go, ge, env = 2, GO, GE, {}
        alphas, betas = list(alphas), list(betas)
        alphas[3] = np.zeros(0, np.uint8)
        betas[9] = np.zeros(0, np.uint8)
    return Subject("score fallback, " + which, env, de.concat(alphas, betas), oracle.align_batch(mode, ASYM, go, ge, alphas, betas, threads=8), mode, ASYM, go, ge, 10000, None)


@pytest.mark.parametrize("which", ["gap_open_positive", "sweep_switched_off", "empty_sequence_highmem"])
def test_score_entry_fallbacks(gpu_lib, monkeypatch, which):
    """off the sweep the score entry runs the align entry's route: the same route number, the same scores, the oracle's"""
    s = _fallback_subject(which)
    apply(monkeypatch, s)
    dev = de.DeviceInputs(s.pb)
    res = de.align(_params(s), dev, _T(s), _T(s))
    accepted(res, s)
    route = _lib.get_timing()["fast_path"]
    rc, scores, guard = de.score(_params(s), dev)
    assert rc == OK and guard
    assert _lib.get_timing()["fast_path"] == route and route not in (7, 8), (route, _lib.get_timing()["fast_path"])
    assert np.array_equal(scores, s.exp[0]) and np.array_equal(scores, res.scores)


def test_score_entry_no_pairs(gpu_lib):
    s = _score_subject("small", 0)
    rc, scores, guard = de.score(_params(s), device(s), n_pairs=0)
    assert rc == OK and scores.shape[0] == 0 and guard  # (with no pairs the guard is the whole buffer: nothing was written)
