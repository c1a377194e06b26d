"""GPU parity of the bulk signature verification (msm_sigs_verify,
msm_sigs_aggregate_verify, msm_sigs_batch_verify, msm_points_in_group;
csrc/sig_verify.hip) on an MI355X.

Oracle: tests/golden/sigs.json, the status codes the reference itself returned
for the tables of tests/sig_inputs.py (blst_core_verify_pk_in_g{1,2} and the
blst_pairing_* sequences).  Every status is compared with the recorded code, not
with the model.
"""
import ctypes
import threading

import pytest

import sig_inputs as si

pytestmark = pytest.mark.gpu

ei = si.ei


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


@pytest.fixture(scope="module")
def fx(golden):
    return golden("sigs.json")


def forms(name):
    out = []
    if name != "individual_encoded":
        out.append("affine")
    if name in si.ENCODED_TOO:
        out.append("encoded")
    return out


def check_table(m, fx, name, scheme, form, what=""):
    call = si.table(name, scheme)
    want = bytes(fx["tables"][name][str(scheme)][form]["status"])
    got = si.run(m, call, form == "encoded")  # (the wrapper asserts nfail == the count of non-zero statuses)
    bad = [j for j in range(len(want)) if got[j:j + 1] != want[j:j + 1]]
    assert not bad and len(got) == len(want), \
        f"{name} scheme {scheme} {form} {what}: check {bad[:1]} got {list(got)} want {list(want)}"


INDIVIDUAL = ["individual", "individual_encoded", "individual_encode", "individual_aug"]
OTHERS = ["key_sets", "aggregate", "batch_w64", "batch_w255", "batch_w0"]


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", INDIVIDUAL)
def test_individual(m, fx, name, scheme):
    for form in forms(name):
        check_table(m, fx, name, scheme, form)


def test_nfail_counts_the_failures(m, fx):
    call = si.table("individual", 1)
    b = si.call_bytes(call)
    n = si.nchecks(call)
    st = (ctypes.c_uint8 * n)()
    nfail = ctypes.c_size_t(0)
    mo = (ctypes.c_size_t * (n + 1))(*b["msg_off"])
    tag = si.tag(1)
    args = (b["keys"], None, b["sigs"], b["msgs"], mo, 0, None, 0, n, tag, len(tag), 0, 0, None)
    m.check(m.lib().msm_sigs_verify(1, 0, st, ctypes.byref(nfail), *args))
    want = fx["tables"]["individual"]["1"]["affine"]["status"]
    assert list(st) == want and nfail.value == sum(1 for v in want if v)
    nfail.value = 0
    m.check(m.lib().msm_sigs_verify(1, 0, None, ctypes.byref(nfail), *args))  # the count alone
    assert nfail.value == sum(1 for v in want if v)


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", OTHERS)
def test_key_sets_aggregates_and_batches(m, fx, name, scheme):
    for form in forms(name):
        check_table(m, fx, name, scheme, form)


@pytest.mark.parametrize("scheme", [1, 2])
def test_every_table_in_chunks_of_16(m, fx, monkeypatch, scheme):
    """chunk cuts fall between checks; the 17-tuple and the 33-tuple checks exceed a chunk"""
    monkeypatch.setenv("MSM_SIGS_CHUNK", "16")
    assert m.lib().msm_sigs_chunk() == 16
    for name in INDIVIDUAL + OTHERS:
        for form in forms(name):
            check_table(m, fx, name, scheme, form, "MSM_SIGS_CHUNK=16")


@pytest.mark.parametrize("piece", ["1", "3"])
def test_pairing_piece_lengths(m, fx, monkeypatch, piece):
    monkeypatch.setenv("MSM_PAIRING_PIECE", piece)
    check_table(m, fx, "batch_w64", 1, "affine", f"MSM_PAIRING_PIECE={piece}")
    check_table(m, fx, "aggregate", 2, "affine", f"MSM_PAIRING_PIECE={piece}")


@pytest.mark.parametrize("group", [1, 2])
def test_in_group(m, group):
    import torch
    pl = si.pool(1)
    good = [pl[i][1] if group == 1 else pl[i][5] for i in range(5)]  # G1: keys of min-pk; G2: its signatures
    pts = good + [None] + [si.off_group(group, i) for i in range(5)] + [ei.GEN[group], None, si.off_group(group, 0)]
    want = bytes([1] * 6 + [0] * 5 + [1, 1, 0])
    raw = b"".join(ei.affine_bytes(group, p) for p in pts)
    keep = bytes(raw)
    assert m.ps_in_group(group, raw, len(pts)) == want
    assert raw == keep
    for p in pts:  # the oracle of the decode tests agrees
        assert ei.in_group(group, ei.affine_bytes(group, p)) == (want[pts.index(p)] == 1)
    dev = torch.device("cuda:0")
    d = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert m.ps_in_group(group, d.data_ptr(), len(pts), src_on_device=True, stream=st.cuda_stream) == want
    st.synchronize()
    assert bytes(d.cpu().numpy()) == keep  # the caller's points are not modified


N_PROP = 33


@pytest.fixture(scope="module")
def signed(m):
    """33 honestly signed tuples made by the library itself (min-pk): keys, messages, signatures"""
    sks = si.mi.gen_scalars(N_PROP, 0x51607)
    sc = b"".join(k.to_bytes(32, "little") for k in sks)
    msgs = [b"message %d" % j for j in range(N_PROP)]
    pk = m.ps_mult(1, ei.affine_bytes(1, ei.GEN[1]), sc, N_PROP, one_point=True)
    hm = m.ps_hash_to_curve(2, msgs, dst_tag=si.tag(1))
    sig = m.ps_mult(2, hm, sc, N_PROP)
    w = b"".join(k.to_bytes(8, "little") for k in si._weights(N_PROP, 64, 0x77e1))
    return sc, msgs, pk, sig, w


def test_batch_names_a_forgery_and_individual_finds_it(m, signed):
    _, msgs, pk, sig, w = signed
    n = N_PROP
    kw = dict(dst_tag=si.tag(1))
    assert m.ps_batch_verify(1, pk, sig, msgs, [0, n], scalars=w, nbits=64, **kw) == b"\x00"
    assert m.ps_verify(1, pk, sig, msgs, **kw) == bytes(n)
    for pos in (0, n // 2, n - 1):
        other = (pos + 1) % n
        forged = sig[:pos * 192] + sig[other * 192:(other + 1) * 192] + sig[(pos + 1) * 192:]
        assert m.ps_batch_verify(1, pk, forged, msgs, [0, n], scalars=w, nbits=64, **kw) == b"\x05"
        assert m.ps_verify(1, pk, forged, msgs, **kw) == bytes(5 if j == pos else 0 for j in range(n))


def test_device_resident_inputs(m, signed):
    """keys, hashes and signatures left in HBM by ps_mult and ps_hash_to_curve on the caller's stream"""
    import torch
    sc, msgs, pk, sig, w = signed
    n = N_PROP
    dev = torch.device("cuda:0")
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    d_sc, d_g1, d_w = up(sc), up(ei.affine_bytes(1, ei.GEN[1])), up(w)
    flat = b"".join(msgs)
    mo = [0]
    for x in msgs:
        mo.append(mo[-1] + len(x))
    d_msgs = up(flat)
    d_pk = torch.zeros(n * 96, dtype=torch.uint8, device=dev)
    d_hm = torch.zeros(n * 192, dtype=torch.uint8, device=dev)
    d_sig = torch.zeros(n * 192, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    kw = dict(dst_tag=si.tag(1), offsets=mo, src_on_device=True)
    with torch.cuda.stream(st):
        s = st.cuda_stream
        m.ps_mult(1, d_g1.data_ptr(), d_sc.data_ptr(), n, one_point=True, src_on_device=True, dst=d_pk.data_ptr(), stream=s)
        m.ps_hash_to_curve(2, d_msgs.data_ptr(), dst_tag=si.tag(1), offsets=mo, src_on_device=True, dst=d_hm.data_ptr(),
                           stream=s)
        m.ps_mult(2, d_hm.data_ptr(), d_sc.data_ptr(), n, src_on_device=True, dst=d_sig.data_ptr(), stream=s)
        got = m.ps_verify(1, d_pk.data_ptr(), d_sig.data_ptr(), d_msgs.data_ptr(), stream=s, **kw)
        d_sig.view(n, 192)[17] = d_sig.view(n, 192)[18]
        bad = m.ps_verify(1, d_pk.data_ptr(), d_sig.data_ptr(), d_msgs.data_ptr(), stream=s, **kw)
        bat = m.ps_batch_verify(1, d_pk.data_ptr(), d_sig.data_ptr(), d_msgs.data_ptr(), [0, 17, n], scalars=d_w.data_ptr(),
                                nbits=64, stream=s, **kw)
        agg = m.ps_aggregate_verify(1, d_pk.data_ptr(), d_sig.data_ptr(), d_msgs.data_ptr(), list(range(n + 1)), stream=s,
                                    **kw)
    st.synchronize()
    host_sig = bytes(d_sig.cpu().numpy())
    hkw = dict(dst_tag=si.tag(1))
    assert got == bytes(n) == m.ps_verify(1, signed[2], signed[3], msgs, **hkw)
    want = bytes(5 if j == 17 else 0 for j in range(n))
    assert bad == want == m.ps_verify(1, signed[2], host_sig, msgs, **hkw)
    assert bat == b"\x00\x05" == m.ps_batch_verify(1, signed[2], host_sig, msgs, [0, 17, n], scalars=w, nbits=64, **hkw)
    assert agg == want == m.ps_aggregate_verify(1, signed[2], host_sig, msgs, list(range(n + 1)), **hkw)
    assert bytes(d_pk.cpu().numpy()) == signed[2]  # the caller's points are left alone


def test_threads_and_engine_cache(m, fx):
    out = [None, None]
    m.release_engine_cache()
    jobs = [("individual", 1, "affine"), ("aggregate", 2, "affine")]

    def work(t):
        name, scheme, form = jobs[t]
        out[t] = si.run(m, si.table(name, scheme), form == "encoded")

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t, (name, scheme, form) in enumerate(jobs):
        assert out[t] == bytes(fx["tables"][name][str(scheme)][form]["status"]), jobs[t]
    out[1] = None
    jobs[1] = ("key_sets", 1, "affine")  # two calls at once on the same (device, scheme) key
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t, (name, scheme, form) in enumerate(jobs):
        assert out[t] == bytes(fx["tables"][name][str(scheme)][form]["status"]), jobs[t]
    live, idle, idle_bytes = m.engine_cache_stats()
    assert idle >= 2 and live >= idle and idle_bytes > 0  # the engines are back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0
