"""What the bulk engines share (csrc/chunk_pipe.hpp: the two staging slots, their
events, the hand-over from one call to the next) on an MI355X, through their
entry points: ps_to_affine, ps_decode, ps_encode, ps_mult, ps_msm_segments and
ps_hash_to_curve, G1 and G2, and the ones that have no group: fr_op, fr_ntt,
fr_eval_quotient, ps_pairing_segments and ps_final_exp.

The expected value of a case is the same call unchunked, host to host, computed
once; the per-operation GPU tests tie that call to the oracles.  Every
comparison is byte for byte.
"""
import pytest

import enc_inputs as ei
import fr_inputs as fi
import h2c_inputs as h
import jac_inputs as ji
import kzg_inputs as ki
import mult_inputs as mi
import pairing_inputs as pi
import seg_inputs as si

pytestmark = pytest.mark.gpu

N = 300  # entries: four chunks of 96 (both slots used twice, the last chunk ragged)
OPS = {"to_affine": "MSM_TO_AFFINE_CHUNK", "decode": "MSM_DECODE_CHUNK", "encode": "MSM_ENCODE_CHUNK",
       "mult": "MSM_POINTS_MULT_CHUNK", "segments": "MSM_POINTS_SEGMENTS_CHUNK", "hash": "MSM_H2C_CHUNK",
       "fr_mul": "MSM_NTT_CHUNK", "fr_inv": "MSM_NTT_CHUNK", "ntt": "MSM_NTT_CHUNK", "poly": "MSM_POLY_CHUNK",
       "pairing": "MSM_PAIRING_CHUNK", "final_exp": "MSM_PAIRING_CHUNK"}
GROUPLESS = ("fr_mul", "fr_inv", "ntt", "poly", "pairing", "final_exp")  # one case each (group None)
LOG_N, BATCH = 5, 10  # ntt, poly: three transforms of 32 per chunk of 96, four chunks, the last of one
PATHS = ["h2h", "h2d", "d2h", "d2d"]  # source memory, destination memory
SEG_LENGTHS = [129, 15, 0, 47, 1, 0, 0, 10, 98]  # 300 points: one segment over three chunks of 96, empty ones
_CASES = {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


class Case:
    """parts: the source buffers (bytes; device runs get them back to back in one
    tensor).  call(srcs, src_on_device, dst, stream) -> (output bytes or None with a
    device dst, further host bytes: the statuses of decode)."""

    def __init__(self, parts, out_len, call):
        self.parts, self.out_len, self.call = parts, out_len, call
        self.want = None


def scalars64(n, seed):
    return mi.scalar_bytes([k & ((1 << 64) - 1) for k in mi.gen_scalars(n, seed)], stride=8, nbytes=8)


def decode_case(m, group, data, n):
    def call(s, dev, dst, stream):
        return m.ps_decode(group, s[0], n, src_on_device=dev, dst=dst, stream=stream)
    return Case([data], n * ei.AFF[group], call)


def segments_case(m, group, lengths, with_scalars=True):
    o = si.offsets_of(lengths)
    n, k = o[-1], len(lengths)
    aff = bytes(m.fixed_points(group, n))
    if not with_scalars:
        return Case([aff], k * ei.AFF[group], lambda s, dev, dst, stream: (
            m.ps_sum_segments(group, s[0], o, src_on_device=dev, dst=dst, stream=stream), b""))
    return Case([aff, scalars64(n, 13)], k * ei.AFF[group], lambda s, dev, dst, stream: (
        m.ps_msm_segments(group, s[0], s[1], o, nbits=64, stride=8, src_on_device=dev, dst=dst, stream=stream), b""))


def build_groupless(m, op):
    F, n = m.FR_BYTES, BATCH << LOG_N
    if op == "fr_mul":
        return Case([fi.pack(fi.rand_values(N, 21)), fi.pack(fi.rand_values(N, 22))], N * F, lambda s, dev, dst, stream: (
            m.fr_op("mul", s[0], s[1], N, src_on_device=dev, dst=dst, stream=stream), b""))
    if op == "fr_inv":  # (adds the level buffer of the batch inversion; a zero among the values)
        vals = fi.special_values()
        return Case([fi.pack(vals + fi.rand_values(N - len(vals), 23))], N * F, lambda s, dev, dst, stream: (
            m.fr_op("inv", s[0], None, N, src_on_device=dev, dst=dst, stream=stream), b""))
    if op == "ntt":
        return Case([fi.pack(fi.rand_values(n, 24))], n * F, lambda s, dev, dst, stream: (
            m.fr_ntt(s[0], LOG_N, BATCH, src_on_device=dev, dst=dst, stream=stream), b""))
    if op == "poly":  # y then q in one output; two of the points lie on the domain
        z = fi.rand_values(BATCH, 26)
        z[3], z[9] = ki.domain(LOG_N)[5], ki.domain(LOG_N)[0]

        def call(s, dev, dst, stream):
            if dst is None:
                y, q = m.fr_eval_quotient(s[0], s[1], LOG_N, BATCH, src_on_device=dev, stream=stream)
                return y + q, b""
            return m.fr_eval_quotient(s[0], s[1], LOG_N, BATCH, src_on_device=dev, y_dst=dst, q_dst=dst + BATCH * F,
                                      stream=stream), b""
        return Case([fi.pack(fi.rand_values(n, 25)), fi.pack(z)], (BATCH + n) * F, call)
    if op == "pairing":
        o = si.offsets_of(SEG_LENGTHS)
        return Case(list(pi.pair_bytes(pi.cyclic(N))), len(SEG_LENGTHS) * m.FP12_BYTES, lambda s, dev, dst, stream: (
            m.ps_pairing_segments(s[0], s[1], o, src_on_device=dev, dst=dst, stream=stream), b""))
    assert op == "final_exp"
    return Case([b"".join(pi.fp12_bytes(f) for f in pi.random_fp12(N, 27))], N * m.FP12_BYTES,
                lambda s, dev, dst, stream: (m.ps_final_exp(s[0], N, src_on_device=dev, dst=dst, stream=stream), b""))


def build(m, op, group):
    if group is None:
        return build_groupless(m, op)
    A = ei.AFF[group]
    aff = bytes(m.fixed_points(group, N))
    if op == "to_affine":
        return Case([ji.jacobians(group, aff, N, 7)], N * A, lambda s, dev, dst, stream: (
            m.ps_to_affine(group, s[0], N, src_on_device=dev, dst=dst, stream=stream), b""))
    if op == "decode":
        return decode_case(m, group, ei.encode(group, aff, N, True), N)
    if op == "encode":
        return Case([aff], N * ei.ENC[group], lambda s, dev, dst, stream: (
            m.ps_encode(group, s[0], N, src_on_device=dev, dst=dst, stream=stream), b""))
    if op == "mult":
        return Case([aff, scalars64(N, 11)], N * A, lambda s, dev, dst, stream: (
            m.ps_mult(group, s[0], s[1], N, nbits=64, stride=8, src_on_device=dev, dst=dst, stream=stream), b""))
    if op == "segments":
        assert sum(SEG_LENGTHS) == N
        return segments_case(m, group, SEG_LENGTHS)
    msgs = h.distinct_messages(N)  # lengths 10 .. 46: the offsets go up with every chunk, whatever the source
    o = si.offsets_of([len(x) for x in msgs])
    return Case([b"".join(msgs)], N * A, lambda s, dev, dst, stream: (
        m.ps_hash_to_curve(group, s[0], offsets=o, dst_tag=h.DST[group], src_on_device=dev, dst=dst, stream=stream), b""))


def expected(case, env, monkeypatch):
    """the call unchunked, host to host; computed once and never modified"""
    if case.want is None:
        monkeypatch.delenv(env, raising=False)
        out, extra = case.call(case.parts, False, None, None)
        assert len(out) == case.out_len
        case.want = (out, extra)
    return case.want


@pytest.fixture
def case(m, request, monkeypatch):
    op, group = request.param
    if (op, group) not in _CASES:
        _CASES[op, group] = build(m, op, group)
    c = _CASES[op, group]
    expected(c, OPS[op], monkeypatch)
    return c, OPS[op]


_PARAMS = [(op, g) for op in OPS for g in ((None,) if op in GROUPLESS else (1, 2))]
ALL = pytest.mark.parametrize("case", _PARAMS, indirect=True,
                              ids=[op if g is None else f"{op}-g{g}" for op, g in _PARAMS])


class Device:
    """torch tensors as the device buffers, and a non-default stream"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(device=self.dev)

    def upload(self, case):
        """the parts back to back in device memory -> their device pointers"""
        t = self.torch.frombuffer(bytearray(b"".join(case.parts)), dtype=self.torch.uint8).to(self.dev)
        ptrs, off = [], 0
        for p in case.parts:
            ptrs.append(t.data_ptr() + off)
            off += len(p)
        return t, ptrs

    def zeros(self, n):
        return self.torch.zeros(n, dtype=self.torch.uint8, device=self.dev)

    def ready(self):
        """the uploads and zeroed buffers (queued on the default stream) are done"""
        self.torch.cuda.synchronize()

    def run(self, case, path):
        """one call on the stream (h2h: on the engine's own) with buffers of its own
        -> (output bytes, further host bytes)"""
        src_dev, dst_dev = path[0] == "d", path[2] == "d"
        d_src = self.upload(case) if src_dev else None
        d_dst = self.zeros(case.out_len) if dst_dev else None
        self.ready()
        stream = self.stream.cuda_stream if path != "h2h" else None
        with self.torch.cuda.stream(self.stream):
            out, extra = case.call(d_src[1] if src_dev else case.parts, src_dev, d_dst.data_ptr() if dst_dev else None,
                                   stream)
        assert (out is None) == dst_dev
        if dst_dev:
            self.stream.synchronize()
            out = bytes(d_dst.cpu().numpy())
        return out, extra


def first_diff(got, want, sz):
    for i in range(len(want) // sz):
        if got[i * sz:(i + 1) * sz] != want[i * sz:(i + 1) * sz]:
            return i
    return None


def assert_same(got, want, what):
    assert len(got[0]) == len(want[0]), what
    assert got[0] == want[0], f"{what}: first differing block of 48 bytes: {first_diff(got[0], want[0], 48)}"
    assert got[1] == want[1], what


@ALL
def test_slot_reuse(m, case, monkeypatch):
    """four chunks through the four memory paths: both slots are used twice and the last chunk is ragged"""
    c, env = case
    monkeypatch.setenv(env, "96")
    d = Device()
    for path in PATHS:
        assert_same(d.run(c, path), c.want, path)


@ALL
def test_regrowth_on_a_pooled_engine(m, case, monkeypatch):
    """one engine, back in the pool between the calls: its pinned and device lanes
    grow from chunks of 32 to chunks of 128 and are then used below their capacity"""
    c, env = case
    m.release_engine_cache()
    for chunk in (32, 128, 32):
        monkeypatch.setenv(env, str(chunk))
        assert_same(c.call(c.parts, False, None, None), c.want, f"chunk {chunk}")
    assert m.engine_cache_stats()[1] >= 1  # the engine went back to the pool every time


@ALL
@pytest.mark.parametrize("src", ["h", "d"])
def test_back_to_back_into_device_destinations(m, case, src, monkeypatch):
    """two calls on one stream with nothing between them (the one synchronisation comes
    before the first): the second is issued while the first is queued or running, waits
    for the engine's last kernel of the first (ev_busy) and for the slots its last chunks
    still hold, and leaves its result alone"""
    c, env = case
    monkeypatch.setenv(env, "96")
    d = Device()
    srcs = d.upload(c) if src == "d" else (None, c.parts)
    d_a, d_b = d.zeros(c.out_len), d.zeros(c.out_len)
    d.ready()
    with d.torch.cuda.stream(d.stream):
        out_a, extra_a = c.call(srcs[1], src == "d", d_a.data_ptr(), d.stream.cuda_stream)
        out_b, extra_b = c.call(srcs[1], src == "d", d_b.data_ptr(), d.stream.cuda_stream)
    assert out_a is None and out_b is None
    d.stream.synchronize()
    assert_same((bytes(d_a.cpu().numpy()), extra_a), c.want, "first call")
    assert_same((bytes(d_b.cpu().numpy()), extra_b), c.want, "second call")


@pytest.mark.parametrize("group", [1, 2])
def test_decode_device_destination_host_status(m, group, monkeypatch):
    """points to device memory, statuses to the host, in chunks, a bad entry in each
    chunk: the path where the status bytes alone come back and are drained"""
    bad = [5, 96, 287, 299]  # chunks of 96: first chunk, first entry of the second, last of the third, the very last
    E = ei.ENC[group]
    enc = bytearray(ei.encode(group, bytes(m.fixed_points(group, N)), N, True))
    off_curve = ei.with_flags(ei.be_bytes(group, ei.OFF_CURVE[group][0]), 0x80)
    for i in bad:
        enc[i * E:(i + 1) * E] = off_curve
    c = decode_case(m, group, bytes(enc), N)
    want = expected(c, OPS["decode"], monkeypatch)
    assert [i for i in range(N) if want[1][i]] == bad
    monkeypatch.setenv(OPS["decode"], "96")
    d = Device()
    for path in ("h2d", "d2d"):
        assert_same(d.run(c, path), want, path)


@pytest.mark.parametrize("group", [1, 2])
def test_segments_empty_at_chunk_boundaries(m, group, monkeypatch):
    """chunks of 48 points and 48 segments: chunks in which no segment ends (nothing
    to copy back, the drain still runs), empty segments where a chunk ends and where
    the next begins, and trailing empty segments that fill chunks of no points at all"""
    lengths = [129, 15, 0, 0, 47, 1, 0, 0, 10, 4] + [0] * 100
    o = si.offsets_of(lengths)
    assert o[2:5] == [144, 144, 144] and o[6:9] == [192, 192, 192]  # 144 = 3 x 48, 192 = 4 x 48
    d = Device()
    for with_scalars in (True, False):
        c = segments_case(m, group, lengths, with_scalars)
        want = expected(c, OPS["segments"], monkeypatch)
        assert want[0][ei.AFF[group] * 10:] == bytes(ei.AFF[group] * 100)  # the empty tail: infinity
        monkeypatch.setenv(OPS["segments"], "48")
        for path in PATHS:
            assert_same(d.run(c, path), want, f"{path}, scalars {with_scalars}")
