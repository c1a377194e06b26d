"""GPU parity of the bulk pairings (msm_pairing_segments, msm_fp12_final_exp;
csrc/pairing.hip) on an MI355X.

Oracle: tests/golden/pairing.json, written from the reference's own
blst_miller_loop / blst_fp12_mul / blst_final_exp: per pair the raw Miller value
and the pairing, per segment layout fe(prod ml) (hex for the first 8 pairs and
every segment, an FNV of the 576 bytes for the rest).  Every value after the
final exponentiation is compared byte for byte; the raw Miller value of the GPU
is pinned only through a final exponentiation (the library's and the model's).
"""
import ctypes
import threading

import pytest

import pairing_inputs as pi

pytestmark = pytest.mark.gpu

G = pi.FP12_BYTES
SIZES = [1, 2, 63, 64, 65, 129]
ALL = list(range(pi.N_PAIRS))


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pairing.json")


def vals(raw):
    assert len(raw) % G == 0
    return [raw[i:i + G] for i in range(0, len(raw), G)]


def check_pairs(got, fx, idx, what=""):
    """got: GT bytes of the pairs idx; the fixture holds hex for the first 8 and an FNV for the rest"""
    got = vals(got)
    assert len(got) == len(idx), (what, len(got), len(idx))
    bad = []
    for k, i in enumerate(idx):
        want = fx["pairs"][i]["e"]
        if (got[k].hex() if len(want) == 2 * G else pi.fnv(got[k])) != want:
            bad.append(k)
    assert not bad, f"{what}: first differing value {bad[0]} (pair {idx[bad[0]]}; {len(bad)} of {len(idx)} differ)"


def offsets_of(layout):
    o = [0]
    for seg in layout:
        o.append(o[-1] + len(seg))
    return o


def flat(layout):
    return [i for seg in layout for i in seg]


def test_pairs_match_the_reference(m, fx):
    p, q = pi.pair_bytes(ALL)
    got = m.ps_pairing(p, q, pi.N_PAIRS)
    check_pairs(got, fx, ALL, "host")
    for i in pi.INF_PAIRS:
        assert vals(got)[i] == m.fp12_one() == pi.fp12_one(), i
    assert m.FP12_BYTES == G


def test_pairs_in_device_memory(m, fx):
    import torch
    dev = torch.device("cuda:0")
    p, q = pi.pair_bytes(ALL)
    d_p = torch.frombuffer(bytearray(p), dtype=torch.uint8).to(dev)
    d_q = torch.frombuffer(bytearray(q), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(pi.N_PAIRS * G, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert m.ps_pairing(d_p.data_ptr(), d_q.data_ptr(), pi.N_PAIRS, src_on_device=True, dst=d_out.data_ptr(),
                            stream=st.cuda_stream) is None
    st.synchronize()
    check_pairs(bytes(d_out.cpu().numpy()), fx, ALL, "device")


def test_final_exp_and_miller_loop_alone(m, fx):
    full = list(range(8))
    ml = bytes.fromhex("".join(fx["pairs"][i]["ml"] for i in full))
    check_pairs(m.ps_final_exp(ml, 8), fx, full, "fe(reference ml)")
    p, q = pi.pair_bytes(ALL)
    raw = m.ps_pairing(p, q, pi.N_PAIRS, final_exp=False)
    check_pairs(m.ps_final_exp(raw, pi.N_PAIRS), fx, ALL, "fe(gpu ml)")
    for i in (0, 5, 23, 24):  # the model's final exponentiation of the raw GPU value
        v = pi.fp12_bytes(pi.final_exp(pi.fp12_from_bytes(vals(raw)[i])))
        check_pairs(v, fx, [i], f"model fe(gpu ml {i})")
    for i in pi.INF_PAIRS:
        assert vals(raw)[i] == pi.fp12_one()


@pytest.mark.parametrize("chunk", [None, "64"])
def test_sizes(m, fx, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MSM_PAIRING_CHUNK", chunk)  # 65 and 129 cross chunk boundaries
    for n in SIZES:
        idx = pi.cyclic(n)
        p, q = pi.pair_bytes(idx)
        check_pairs(m.ps_pairing(p, q, n), fx, idx, f"n={n} chunk={chunk}")


def run_layout(m, fx, name):
    layout = pi.SEGMENTS[name]
    p, q = pi.pair_bytes(flat(layout))
    o = offsets_of(layout)
    got = m.ps_pairing_segments(p, q, o)
    want = bytes.fromhex("".join(fx["segments"][name]))
    bad = [j for j in range(len(layout)) if got[j * G:(j + 1) * G] != want[j * G:(j + 1) * G]]
    assert not bad and len(got) == len(want), f"{name}: first differing segment {bad[:1]} of lengths {[len(s) for s in layout]}"
    verdict = m.ps_pairing_check(p, q, o)
    assert verdict == bytes(1 if v == pi.fp12_one() else 0 for v in vals(want)), name
    return got


@pytest.mark.parametrize("piece,name", [(None, "L1"), (None, "L3"), ("1", "L1"), ("3", "L3"), ("3", "L1"), ("1", "L3")])
def test_segment_layouts(m, fx, monkeypatch, piece, name):
    if piece:
        monkeypatch.setenv("MSM_PAIRING_PIECE", piece)
    got = run_layout(m, fx, name)
    assert vals(got)[0] == vals(got)[-1] == pi.fp12_one()  # the empty segments


@pytest.mark.parametrize("piece", [None, "3", "64"])
def test_segment_spanning_chunks(m, fx, monkeypatch, piece):
    monkeypatch.setenv("MSM_PAIRING_CHUNK", "64")
    if piece:
        monkeypatch.setenv("MSM_PAIRING_PIECE", piece)
    run_layout(m, fx, "span100")


@pytest.mark.parametrize("piece", [None, "3"])
def test_infinity_inside_segments(m, fx, monkeypatch, piece):
    if piece:
        monkeypatch.setenv("MSM_PAIRING_PIECE", piece)
    run_layout(m, fx, "inf_ends")
    assert run_layout(m, fx, "inf_only") == pi.fp12_one()


def test_segment_against_its_halves(m):
    seg = [0, 1, 2, 3, 4, 5, 6]
    p, q = pi.pair_bytes(seg)
    whole = m.ps_pairing_segments(p, q, [0, 7])
    halves = vals(m.ps_pairing_segments(p, q, [0, 3, 7], final_exp=False))
    prod = pi.f12_mul(pi.fp12_from_bytes(halves[0]), pi.fp12_from_bytes(halves[1]))
    assert pi.fp12_bytes(pi.final_exp(prod)) == whole
    assert m.ps_final_exp(pi.fp12_bytes(prod), 1) == whole


def test_bilinear_through_the_library(m):
    n = 8
    ks = pi.mi.gen_scalars(n, 0xb111)
    sc = b"".join(k.to_bytes(32, "little") for k in ks)
    idx = list(range(n))
    p, q = pi.pair_bytes(idx)
    ap = m.ps_mult(1, p, sc, n)
    aq = m.ps_mult(2, q, sc, n)
    left, right = m.ps_pairing(ap, q, n), m.ps_pairing(p, aq, n)
    assert left == right
    assert len(set(vals(left))) == n and pi.fp12_one() not in vals(left)
    # e(P, Q) e(-P, Q) = 1
    P0, Q0 = pi.pairs()[0]
    neg = pi.ei.affine_bytes(1, (P0[0], -P0[1] % pi.P))
    pp, qq = pi.ei.affine_bytes(1, P0) + neg, pi.ei.affine_bytes(2, Q0) * 2
    assert m.ps_pairing_segments(pp, qq, [0, 2]) == pi.fp12_one()
    assert m.ps_pairing_check(pp, qq, [0, 2]) == b"\x01"
    assert m.ps_pairing_check(pp, qq, [0, 1, 2]) == b"\x00\x00"


N_SIG = 33


def test_signature_check_end_to_end(m):
    import torch
    dev = torch.device("cuda:0")
    n = N_SIG
    sks = pi.mi.gen_scalars(n, 0x51607)
    sc = b"".join(k.to_bytes(32, "little") for k in sks)
    msgs = [b"message %d" % j for j in range(n)]
    tag = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"
    g1 = pi.ei.affine_bytes(1, pi.G1)
    pk = m.ps_mult(1, g1, sc, n, one_point=True)
    hm = m.ps_hash_to_curve(2, msgs, dst_tag=tag)
    sig = m.ps_mult(2, hm, sc, n)
    neg = pi.neg_g1()

    def interleave(a, b, size):
        return b"".join(a[j * size:(j + 1) * size] + b[j * size:(j + 1) * size] for j in range(n))

    o = list(range(0, 2 * n + 1, 2))
    p = interleave(pk, neg * n, 96)
    assert m.ps_pairing_check(p, interleave(hm, sig, 192), o) == b"\x01" * n
    forged = sig[:17 * 192] + sig[18 * 192:19 * 192] + sig[18 * 192:]
    q_bad = interleave(hm, forged, 192)
    want = bytes(0 if j == 17 else 1 for j in range(n))
    assert m.ps_pairing_check(p, q_bad, o) == want
    verdict = (ctypes.c_uint8 * n)()
    nfail = ctypes.c_size_t(99)
    m.check(m.lib().msm_pairing_segments(0, None, verdict, ctypes.byref(nfail), p, q_bad, (ctypes.c_size_t * (n + 1))(*o),
                                         n, 0, 0, 0, None))
    assert bytes(verdict) == want and nfail.value == 1
    # the same with every input left on the device from the calls that produced it
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    d_g1 = torch.frombuffer(bytearray(g1), dtype=torch.uint8).to(dev)
    d_neg = torch.frombuffer(bytearray(neg), dtype=torch.uint8).to(dev)
    d_p = torch.zeros(n, 2, 96, dtype=torch.uint8, device=dev)
    d_q = torch.zeros(n, 2, 192, dtype=torch.uint8, device=dev)
    d_pk = torch.zeros(n * 96, dtype=torch.uint8, device=dev)
    d_hm = torch.zeros(n * 192, dtype=torch.uint8, device=dev)
    d_sig = torch.zeros(n * 192, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s = st.cuda_stream
        m.ps_mult(1, d_g1.data_ptr(), d_sc.data_ptr(), n, one_point=True, src_on_device=True, dst=d_pk.data_ptr(), stream=s)
        m.ps_hash_to_curve(2, msgs, dst_tag=tag, dst=d_hm.data_ptr(), stream=s)
        m.ps_mult(2, d_hm.data_ptr(), d_sc.data_ptr(), n, src_on_device=True, dst=d_sig.data_ptr(), stream=s)
        d_p[:, 0] = d_pk.view(n, 96)
        d_p[:, 1] = d_neg
        d_q[:, 0] = d_hm.view(n, 192)
        d_q[:, 1] = d_sig.view(n, 192)
        assert m.ps_pairing_check(d_p.data_ptr(), d_q.data_ptr(), o, src_on_device=True, stream=s) == b"\x01" * n
        d_q[17, 1] = d_sig.view(n, 192)[18]
        assert m.ps_pairing_check(d_p.data_ptr(), d_q.data_ptr(), o, src_on_device=True, stream=s) == want
    st.synchronize()


def test_threads_and_engine_cache(m, fx):
    out = [None, None]
    m.release_engine_cache()
    idx = [list(range(0, 14)), list(range(14, pi.N_PAIRS))]

    def work(t):
        p, q = pi.pair_bytes(idx[t])
        out[t] = m.ps_pairing(p, q, len(idx[t]))

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(2):
        assert out[t] is not None
        check_pairs(out[t], fx, idx[t], f"thread {t}")
    live, idle, idle_bytes = m.engine_cache_stats()
    assert idle >= 1 and live >= idle and idle_bytes > 0  # the engines are back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0


# ---- the final exponentiation at its edges (msm_fp12_final_exp on arbitrary input) ----
def special_bytes(names):
    sp = pi.special_fp12()
    return b"".join(pi.fp12_bytes(sp[k]) for k in names)


def special_want(fx, names):
    return bytes.fromhex("".join(fx["tower"]["values"][k]["final_exp"] for k in names))


def fe_verdicts(m, src, n):
    """(values, is_one bytes, nfail) of one msm_fp12_final_exp call on host memory"""
    out = (ctypes.c_uint8 * (n * G))()
    verdict = (ctypes.c_uint8 * n)(*([7] * n))
    nfail = ctypes.c_size_t(99)
    m.check(m.lib().msm_fp12_final_exp(0, out, verdict, ctypes.byref(nfail), src, n, 0, 0, None))
    return bytes(out), bytes(verdict), nfail.value


def test_final_exp_special_values_and_verdicts(m, fx):
    """subfield elements, roots of one, the sparse shape of a line, all-maximal coordinates:
    values byte for byte the reference's, and the verdict path on values that are exactly
    one for another reason than an empty or cancelling segment"""
    names = pi.SPECIAL_NAMES
    src, want = special_bytes(names), special_want(fx, names)
    got = m.ps_final_exp(src, len(names))
    bad = [names[i] for i in range(len(names)) if vals(got)[i] != vals(want)[i]]
    assert not bad, f"final exponentiation differs from the reference on {bad}"
    ones = bytes(1 if v == pi.fp12_one() else 0 for v in vals(want))
    assert ones == bytes(1 if k in pi.SPECIAL_FE_ONE else 0 for k in names) and sum(ones) == 8
    out, verdict, nfail = fe_verdicts(m, src, len(names))
    assert out == want and verdict == ones and nfail == len(names) - sum(ones)
    # the verdicts alone (no values wanted)
    verdict = (ctypes.c_uint8 * len(names))()
    m.check(m.lib().msm_fp12_final_exp(0, None, verdict, None, src, len(names), 0, 0, None))
    assert bytes(verdict) == ones


def test_final_exp_zero_among_its_neighbours(m, fx):
    """the all-zero value at slots 0, 31 and 64 of 65: the call returns MSM_OK, every other
    slot is right, and the zero slots give zero, not one, as the reference's blst_final_exp
    does (straight-line arithmetic: the Fermat chain of a zero norm is zero)"""
    assert fx["tower"]["final_exp_of_zero_is_zero"] is True
    n, zeros = 65, (0, 31, 64)
    names = [pi.SPECIAL_NAMES[i % 13] for i in range(n)]
    rnd = pi.random_fp12(8, 0xfe0)
    src, want = [], []
    for i in range(n):
        if i in zeros:
            src.append(bytes(G))
            want.append(bytes(G))
        elif i % 8 == 5:
            src.append(pi.fp12_bytes(rnd[i // 8]))
            want.append(pi.fp12_bytes(pi.final_exp(rnd[i // 8])))
        else:
            src.append(special_bytes([names[i]]))
            want.append(special_want(fx, [names[i]]))
    out, verdict, nfail = fe_verdicts(m, b"".join(src), n)
    got = vals(out)
    bad = [i for i in range(n) if i not in zeros and got[i] != want[i]]
    assert not bad, f"non-zero slots {bad} differ beside a zero input"
    assert [got[i] == bytes(G) for i in zeros] == [True] * 3, "fe(0) is not zero"
    ones = bytes(1 if w == pi.fp12_one() else 0 for w in want)
    assert verdict == ones and nfail == n - sum(ones) and all(verdict[i] == 0 for i in zeros)


@pytest.mark.parametrize("chunk", [None, "64"])
def test_final_exp_special_values_at_sizes(m, fx, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MSM_PAIRING_CHUNK", chunk)  # 65 and 129 cross chunk boundaries
    for n in [1, 63, 64, 65, 129]:
        names = [pi.SPECIAL_NAMES[(i + n) % 13] for i in range(n)]
        want = special_want(fx, names)
        out, verdict, nfail = fe_verdicts(m, special_bytes(names), n)
        bad = [i for i in range(n) if vals(out)[i] != vals(want)[i]]
        assert not bad, f"n={n} chunk={chunk}: slots {bad[:8]} differ"
        ones = bytes(1 if k in pi.SPECIAL_FE_ONE else 0 for k in names)
        assert verdict == ones and nfail == n - sum(ones), (n, chunk)


def test_final_exp_special_values_in_device_memory(m, fx):
    import torch
    dev = torch.device("cuda:0")
    names = pi.SPECIAL_NAMES
    d_src = torch.frombuffer(bytearray(special_bytes(names)), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(len(names) * G, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert m.ps_final_exp(d_src.data_ptr(), len(names), src_on_device=True, dst=d_out.data_ptr(),
                              stream=st.cuda_stream) is None
    st.synchronize()
    assert bytes(d_out.cpu().numpy()) == special_want(fx, names)
