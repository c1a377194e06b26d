"""msm_blst_amd -- MI355X-native BLS12-381 multi-scalar multiplication.

Host-side Python mirror of the reference's MSM interface (LuoGuiwen/MSM_blst,
a blst v0.3.10 fork).  The compute runs in hand-written HIP kernels for
gfx950 inside libmsm_mi355x.so (include/msm_mi355x.h); this module only
moves bytes and calls the C ABI.

Mirrors:
  blst_p1s_mult_pippenger / blst_p2s_mult_pippenger  (ref bindings/blst.h:238-246, :377-384)
  MSMContext                                          device-resident points (extension)
  ches.CHESContext                                    ref main_p1.cpp CHES driver (see ches.py)
  bgmw.BGMWContext                                    ref main_p1.cpp BGMW95 driver (see bgmw.py)
  wbits.WbitsContext, wbits.precompute / wbits.mult   blst_p{1,2}s_mult_wbits[_precompute] (see wbits.py)
  ps_to_affine                                        blst_p{1,2}s_to_affine (ref multi_scalar.c:17-62), bulk, on the GPU
  ps_decode, MSMContext.set_points_encoded            blst_p{1,2}_uncompress / _deserialize / _affine_in_g{1,2}
                                                      (ref e1.c:236-351, e2.c:279-410), bulk, on the GPU
  ps_mult                                             out[i] = [k_i]P_i: a loop over blst_p{1,2}_mult / _unchecked_mult
                                                      (ref e1.c:505-533, ec_mult.h), bulk, on the GPU
  ps_encode                                           blst_p{1,2}_[affine_]compress / _serialize (ref e1.c:139-234,
                                                      e2.c), bulk, on the GPU
  ps_msm_segments, ps_sum_segments                    k MSMs / k sums over k point sets in one call: a loop over
                                                      blst_p{1,2}s_mult_pippenger / blst_p{1,2}s_add per set (ref
                                                      multi_scalar.c:581-607, bulk_addition.c:145-164), on the GPU
  ps_hash_to_curve, ps_hash_to_field, ps_map_to_curve blst_hash_to_g{1,2} / blst_encode_to_g{1,2} / blst_map_to_g{1,2} and
                                                      hash_to_field (ref map_to_g1.c:285-453, map_to_g2.c:173-401,
                                                      hash_to_field.c:51-154), bulk, on the GPU
  ps_pairing, ps_pairing_segments, ps_pairing_check,  blst_miller_loop / blst_fp12_mul / blst_final_exp / blst_fp12_is_one
  ps_final_exp                                        (ref pairing.c:181-262, 371-404), bulk, on the GPU
  ps_verify, ps_aggregate_verify, ps_batch_verify,    blst_core_verify_pk_in_g{1,2} and the blst_pairing_chk_n_[mul_n_]aggr_pk_in_g{1,2}
  ps_in_group                                         / commit / finalverify sequences (ref aggregate.c), blst_p{1,2}_affine_in_g{1,2},
                                                      bulk, on the GPU
  fr_ntt, fr_op, fr_root_of_unity, ntt_plan            batched NTTs over Fr and the loops over blst_fr_add / _sub / _mul /
                                                      _sqr / _cneg / _inverse / _from_scalar / blst_scalar_from_fr (ref
                                                      exports.c), bulk, on the GPU
  fr_eval_quotient                                    f(z) and (f - f(z)) / (X - z) of evaluation-form polynomials (no
                                                      reference counterpart: the loop a KZG prover writes over blst_fr_*)
  KZGContext                                          commit / open / verify over a Lagrange-form SRS: the chain of
                                                      blst_p1s_mult_pippenger, blst_p1_mult and blst_miller_loop /
                                                      blst_final_exp calls of a KZG prover and verifier, on the GPU;
                                                      KZGContext.from_monomial builds it from powers of tau
  ps_ntt, ntt_model                                   NTTs over G1 / G2 points (no reference counterpart: the loop over
                                                      blst_p{1,2}_mult and blst_p{1,2}_add_or_double that changes the basis
                                                      of an SRS), on the GPU, and the host model of their schedule
"""
import ctypes

from ._ffi import MsmError, check, lib
from .bgmw import BGMWContext
from .ches import CHESContext
from .wbits import WbitsContext

__all__ = ["MsmError", "MSMContext", "CHESContext", "BGMWContext", "WbitsContext", "p1s_mult_pippenger", "p2s_mult_pippenger", "ps_add", "fixed_points", "gen_scalars",
           "compress", "to_affine", "ps_to_affine", "to_affine_levels", "ps_decode", "ps_mult", "ps_encode",
           "ps_msm_segments", "ps_sum_segments", "segments_plan",
           "ps_map_to_curve", "ps_hash_to_field", "ps_hash_to_curve", "h2c_dst_prime",
           "ps_pairing", "ps_pairing_segments", "ps_pairing_check", "ps_final_exp", "fp12_one", "FP12_BYTES",
           "ps_verify", "ps_aggregate_verify", "ps_batch_verify", "ps_in_group", "sigs_plan", "sigs_reduce",
           "SIG_MIN_PK", "SIG_MIN_SIG",
           "fr_ntt", "fr_op", "fr_root_of_unity", "ntt_plan", "fr_probe", "FR_OPS",
           "fr_eval_quotient", "KZGContext", "POLY_BITREV", "ps_ntt", "ntt_model",
           "SRC_AFFINE", "SRC_JACOBIAN", "device_count", "lib"]

POINT_BYTES = {1: 96, 2: 192}
JAC_BYTES = {1: 144, 2: 288}
ENC_COMPRESSED, ENC_SERIALIZED = 0, 1  # MSM_ENC_*: 48 G / 96 G bytes per entry
DECODE_CHECK_GROUP = 1                 # MSM_DECODE_CHECK_GROUP
MULT_ONE_POINT = 1                     # MSM_MULT_ONE_POINT
SRC_AFFINE, SRC_JACOBIAN = 0, 1        # MSM_SRC_*: 96 G / 144 G bytes per point
H2C_ENCODE = 1                         # MSM_H2C_ENCODE
PAIRING_MILLER_ONLY = 1                # MSM_PAIRING_MILLER_ONLY
FP12_BYTES = 576                       # a GT value: blst_fp12
SIG_MIN_PK, SIG_MIN_SIG = 1, 2         # MSM_SIG_*: the group of the public keys
SIG_ENCODED = 2                        # MSM_SIG_ENCODED
NTT_INVERSE, FR_SRC_SCALAR, FR_DST_SCALAR = 1, 2, 4  # MSM_NTT_INVERSE, MSM_FR_{SRC,DST}_SCALAR
FR_B_ONE = 1                           # MSM_FR_B_ONE
POLY_BITREV = 8                        # MSM_POLY_BITREV: positions in bit-reversed order
FR_BYTES = 32                          # a blst_fr or a blst_scalar
# MSM_FR_*: the ops of fr_op, by name
FR_OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "inv": 5, "from_scalar": 6, "to_scalar": 7}


def device_count():
    return lib().msm_device_count()


def engine_cache_stats():
    """(engines alive, idle, device bytes of idle engines) of the pool behind the
    blst-named entry points (include/msm_mi355x.h msm_engine_cache_stats)."""
    out = (ctypes.c_size_t * 3)()
    lib().msm_engine_cache_stats(out)
    return tuple(out)


def release_engine_cache():
    lib().msm_release_engine_cache()


def set_engine_cache_limit(nbytes):
    return lib().msm_set_engine_cache_limit(nbytes)


def _buf(data):
    if isinstance(data, (bytes, bytearray)):
        return (ctypes.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    return data


def gen_scalars(n, seed):
    """n 32-byte little-endian scalars < r (SplitMix64)."""
    out = (ctypes.c_uint8 * (32 * n))()
    lib().msm_gen_scalars(out, n, seed)
    return out


def fixed_points(group, n, start=0):
    """P_i = 2^(i+1) G for i in [start, start+n) (ref main_p1.cpp:52-66), blst affine layout."""
    out = (ctypes.c_uint8 * (POINT_BYTES[group] * n))()
    getattr(lib(), f"msm_p{group}_fixed_points_range")(out, start, n)
    return out


def compress(group, jac):
    out = (ctypes.c_uint8 * (48 * group))()
    getattr(lib(), f"msm_p{group}_compress")(out, _buf(jac))
    return bytes(out)


def to_affine(group, jac):
    out = (ctypes.c_uint8 * POINT_BYTES[group])()
    getattr(lib(), f"msm_p{group}_to_affine")(out, _buf(jac))
    return bytes(out)


def ps_to_affine(group, jacobians, n, *, src_on_device=False, dst=None, device=0, stream=None):
    """n Jacobians (blst_p1 / blst_p2 layout, 144 / 288 B each) -> n affine points
    (msm_points_to_affine; Z = 0 gives the all-zero point).  A host source is a
    bytes-like object, a device source (src_on_device) a device pointer.  Without
    dst the result comes back as bytes; with dst=<device pointer> it is written
    there, ordered on `stream`, and None is returned."""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if n < 0:
        raise ValueError("n must be >= 0")
    if src_on_device:
        src = jacobians
    else:
        src = _buf(jacobians)
        have = len(src) if hasattr(src, "__len__") else ctypes.sizeof(src)
        if have < n * JAC_BYTES[group]:
            raise ValueError(f"{have} bytes of Jacobians given, {n * JAC_BYTES[group]} needed")
    if dst is not None:
        check(lib().msm_points_to_affine(group, device, dst, src, n, int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * (POINT_BYTES[group] * n))()
    check(lib().msm_points_to_affine(group, device, out, src, n, int(bool(src_on_device)), 0, stream))
    return bytes(out)


def _encoded(group, data, n, compressed, on_device):
    """(pointer or ctypes buffer, encoding) of n encoded entries; a short host buffer raises"""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if n < 0:
        raise ValueError("n must be >= 0")
    if on_device:
        return data, ENC_COMPRESSED if compressed else ENC_SERIALIZED
    src = _buf(data)
    have = len(src) if hasattr(src, "__len__") else ctypes.sizeof(src)
    need = n * 48 * group * (1 if compressed else 2)
    if have < need:
        raise ValueError(f"{have} bytes of encoded points given, {need} needed")
    return src, ENC_COMPRESSED if compressed else ENC_SERIALIZED


def ps_decode(group, data, n, *, compressed=True, check_group=True, src_on_device=False, dst=None, device=0,
              stream=None):
    """n ZCash-encoded points (48 G bytes each compressed, 96 G serialized) -> (affine
    bytes, status bytes) through msm_points_decode: status 0 ok, 1 bad encoding, 2 not
    on the curve, 3 not in the group; the affine point of every failed entry is all
    zero.  check_group adds the subgroup test.  A host source is a bytes-like object,
    a device source (src_on_device) a device pointer.  With dst=<device pointer> the
    points are written there, ordered on `stream`, and (None, status bytes) is returned."""
    src, enc = _encoded(group, data, n, compressed, src_on_device)
    flags = DECODE_CHECK_GROUP if check_group else 0
    status = (ctypes.c_uint8 * n)()
    if dst is not None:
        check(lib().msm_points_decode(group, device, dst, status, None, src, n, enc, flags, int(bool(src_on_device)), 1,
                                      stream))
        return None, bytes(status)
    out = (ctypes.c_uint8 * (POINT_BYTES[group] * n))()
    check(lib().msm_points_decode(group, device, out, status, None, src, n, enc, flags, int(bool(src_on_device)), 0,
                                  stream))
    return bytes(out), bytes(status)


def ps_mult(group, points, scalars, n, *, nbits=255, stride=32, one_point=False, src_on_device=False, dst=None,
            device=0, stream=None):
    """out[i] = [k_i] P_i for i < n as affine bytes (msm_points_mult; infinity is the
    all-zero point).  points: n affine points, or ONE with one_point (fixed base).
    k_i: the low nbits bits of the little-endian scalar at scalars[i * stride:]; bits
    above nbits in the last byte are ignored.  The result is exact for every point of
    the curve, subgroup or not.  Host sources are bytes-like objects, device sources
    (src_on_device, both) device pointers.  With dst=<device pointer> the points are
    written there, ordered on `stream`, and None is returned."""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if n < 0:
        raise ValueError("n must be >= 0")
    if not 0 <= nbits <= 256:
        raise ValueError("nbits must be in [0, 256]")
    nb = (nbits + 7) // 8
    if stride < nb:
        raise ValueError(f"stride {stride} shorter than the {nb} bytes of a {nbits}-bit scalar")
    if src_on_device:
        pts, sc = points, scalars
    else:
        pts, sc = _buf(points), _buf(scalars)
        have = len(pts) if hasattr(pts, "__len__") else ctypes.sizeof(pts)
        need = POINT_BYTES[group] * (min(n, 1) if one_point else n)
        if have < need:
            raise ValueError(f"{have} bytes of points given, {need} needed")
        have = len(sc) if hasattr(sc, "__len__") else ctypes.sizeof(sc)
        need = (n - 1) * stride + nb if n else 0
        if have < need:
            raise ValueError(f"{have} bytes of scalars given, {need} needed")
    flags = MULT_ONE_POINT if one_point else 0
    if dst is not None:
        check(lib().msm_points_mult(group, device, dst, pts, sc, n, nbits, stride, flags, int(bool(src_on_device)), 1,
                                    stream))
        return None
    out = (ctypes.c_uint8 * (POINT_BYTES[group] * n))()
    check(lib().msm_points_mult(group, device, out, pts, sc, n, nbits, stride, flags, int(bool(src_on_device)), 0,
                                stream))
    return bytes(out)


def ps_encode(group, points, n, *, compressed=True, jacobian=False, src_on_device=False, dst=None, device=0,
              stream=None):
    """n affine points (96 G bytes each), or Jacobians (144 G bytes, jacobian=True), ->
    n ZCash entries of 48 G bytes (compressed) or 96 G bytes through msm_points_encode,
    byte for byte what blst_p{1,2}_[affine_]compress / _serialize give.  Nothing is
    validated; the all-zero affine point and every Jacobian with Z = 0 are infinity.
    A host source is a bytes-like object, a device source (src_on_device) a device
    pointer.  Without dst the entries come back as bytes; with dst=<device pointer>
    they are written there, ordered on `stream`, and None is returned."""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if n < 0:
        raise ValueError("n must be >= 0")
    form = SRC_JACOBIAN if jacobian else SRC_AFFINE
    enc = ENC_COMPRESSED if compressed else ENC_SERIALIZED
    if src_on_device:
        src = points
    else:
        src = _buf(points)
        have = len(src) if hasattr(src, "__len__") else ctypes.sizeof(src)
        need = n * (JAC_BYTES if jacobian else POINT_BYTES)[group]
        if have < need:
            raise ValueError(f"{have} bytes of points given, {need} needed")
    if dst is not None:
        check(lib().msm_points_encode(group, device, dst, src, n, form, enc, 0, int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * (n * 48 * group * (1 if compressed else 2)))()
    check(lib().msm_points_encode(group, device, out, src, n, form, enc, 0, int(bool(src_on_device)), 0, stream))
    return bytes(out)


def _fr_host(data, need, what):
    src = _buf(data)
    have = len(src) if hasattr(src, "__len__") else ctypes.sizeof(src)
    if have < need:
        raise ValueError(f"{have} bytes of {what} given, {need} needed")
    return src


def fr_ntt(data, log_n, batch=1, *, inverse=False, shift=None, src_scalar=False, dst_scalar=False,
           src_on_device=False, dst=None, device=0, stream=None):
    """`batch` transforms of 2^log_n Fr elements each (32 bytes: blst_fr, or blst_scalar
    with src_scalar / dst_scalar) through msm_fr_ntt, natural order in and out:
    forward dst[k] = sum_j src[j] omega_n^(j k), inverse dst[j] = n^-1 sum_k src[k]
    omega_n^(-j k).  shift: None or s in (0, r), an int or 32 little-endian bytes; the
    forward transform evaluates on the coset s <omega_n>, the inverse undoes it.  A
    host source is a bytes-like object, a device source (src_on_device) a device
    pointer.  Without dst the result comes back as bytes; with dst=<device pointer>
    (which may be the source) it is written there, ordered on `stream`, and None is
    returned."""
    if not 0 <= log_n <= 26:
        raise ValueError("log_n must be in [0, 26]")
    if batch < 0:
        raise ValueError("batch must be >= 0")
    nbytes = (batch << log_n) * FR_BYTES
    src = data if src_on_device else _fr_host(data, nbytes, "elements")
    if shift is not None:
        if isinstance(shift, int):
            if not 0 < shift < (1 << 256):
                raise ValueError("shift must be in (0, r)")
            shift = shift.to_bytes(32, "little")
        shift = _fr_host(shift, 32, "shift")
    flags = (NTT_INVERSE if inverse else 0) | (FR_SRC_SCALAR if src_scalar else 0) | (FR_DST_SCALAR if dst_scalar else 0)
    if dst is not None:
        check(lib().msm_fr_ntt(device, dst, src, log_n, batch, shift, flags, int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * nbytes)()
    check(lib().msm_fr_ntt(device, out, src, log_n, batch, shift, flags, int(bool(src_on_device)), 0, stream))
    return bytes(out)


def fr_op(op, a, b=None, n=None, *, b_one=False, src_on_device=False, dst=None, device=0, stream=None):
    """dst[i] = a[i] op b[i] for i < n through msm_fr_op, byte for byte what the
    reference's blst_fr_* give.  op: a name of FR_OPS ("add", "sub", "mul", "sqr",
    "neg", "inv", "from_scalar", "to_scalar") or its number; b is read by add, sub and
    mul only, and with b_one it holds ONE element used for every a[i].  The inverse
    of zero is zero.  n defaults to the elements of a host `a`.  Host sources are
    bytes-like objects, device sources (src_on_device, both) device pointers; with
    dst=<device pointer> (which may be a or b) the result is written there, ordered on
    `stream`, and None is returned."""
    code = FR_OPS[op] if isinstance(op, str) else int(op)
    two = code in (0, 1, 2)
    if two and b is None:
        raise ValueError("this op needs b")
    if n is None:
        if src_on_device:
            raise ValueError("n must be given with device sources")
        n = len(a) // FR_BYTES
    if n < 0:
        raise ValueError("n must be >= 0")
    if src_on_device:
        pa, pb = a, b
    else:
        pa = _fr_host(a, n * FR_BYTES, "a")
        pb = _fr_host(b, (min(n, 1) if b_one else n) * FR_BYTES, "b") if two else None
    flags = FR_B_ONE if b_one else 0
    if dst is not None:
        check(lib().msm_fr_op(device, code, dst, pa, pb, n, flags, int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * (n * FR_BYTES))()
    check(lib().msm_fr_op(device, code, out, pa, pb, n, flags, int(bool(src_on_device)), 0, stream))
    return bytes(out)


def fr_root_of_unity(log_n):
    """omega_n for n = 2^log_n (log_n <= 32) as the 32 bytes of a blst_fr; omega_(2^32) =
    7^((r - 1) / 2^32)."""
    out = (ctypes.c_uint8 * FR_BYTES)()
    check(lib().msm_fr_root_of_unity(log_n, out))
    return bytes(out)


def ntt_plan(log_n):
    """log2 of the radix of every pass of a 2^log_n transform, under the MSM_NTT_TILE set
    now (msm_ntt_plan; empty for log_n = 0)."""
    n = ctypes.c_int(0)
    radix = (ctypes.c_int * 32)()
    check(lib().msm_ntt_plan(log_n, ctypes.byref(n), radix, 32))
    return list(radix[:n.value])


def fr_probe(device=0):
    """(register-resident Fr products per second, milliseconds measured) on `device`."""
    out = (ctypes.c_double * 2)()
    check(lib().msm_fr_probe(device, out))
    return out[0], out[1]


def fr_eval_quotient(polys, z, log_n, count=1, *, want_q=True, dst_scalar=False, bitrev=False, src_on_device=False,
                     y_dst=None, q_dst=None, device=0, stream=None):
    """`count` polynomials of 2^log_n blst_fr each, given by their values on the domain
    of fr_ntt (position i: the value at omega_n^i, or with bitrev at omega_n^bitrev(i)),
    and one blst_fr point z[j] per polynomial, through msm_fr_eval_quotient: y[j] = f_j(z[j])
    and, with want_q, the values of (f_j - y_j) / (X - z_j) on the same domain in the
    same order (blst_fr, or blst_scalar bytes with dst_scalar).  Host sources are
    bytes-like objects, device sources (src_on_device, both) device pointers.  Returns
    (y, q) as bytes (q None without want_q); with y_dst=<device pointer> (and q_dst,
    which may be the source, when q is wanted) the results are written there, ordered
    on `stream`, and None is returned."""
    if not 0 <= log_n <= 26:
        raise ValueError("log_n must be in [0, 26]")
    if count < 0:
        raise ValueError("count must be >= 0")
    nbytes = (count << log_n) * FR_BYTES
    if src_on_device:
        pp, pz = polys, z
    else:
        pp, pz = _fr_host(polys, nbytes, "polynomial values"), _fr_host(z, count * FR_BYTES, "points")
    flags = (FR_DST_SCALAR if dst_scalar else 0) | (POLY_BITREV if bitrev else 0)
    sd = int(bool(src_on_device))
    if y_dst is not None:
        if want_q and q_dst is None:
            raise ValueError("q_dst must be given with y_dst when the quotient is wanted")
        check(lib().msm_fr_eval_quotient(device, y_dst, q_dst if want_q else None, pp, pz, log_n, count, flags, sd, 1,
                                         stream))
        return None
    y = (ctypes.c_uint8 * max(count * FR_BYTES, 1))()
    q = (ctypes.c_uint8 * max(nbytes, 1))() if want_q else None
    check(lib().msm_fr_eval_quotient(device, y, q, pp, pz, log_n, count, flags, sd, 0, stream))
    return bytes(y)[:count * FR_BYTES], (bytes(q)[:nbytes] if want_q else None)


def ps_ntt(group, points, log_n, batch=1, *, inverse=False, bitrev=False, src_on_device=False, dst=None, device=0,
           stream=None):
    """`batch` transforms of 2^log_n affine points each through msm_points_ntt, on the
    domain of fr_ntt: forward dst[k] = sum_j [omega_n^(j k)] src[j], inverse dst[j] =
    [n^-1] sum_k [omega_n^(-j k)] src[k].  bitrev puts the evaluation side in bit-reversed
    order (the inverse writes result j at bitrev(j), the forward transform reads element j
    at bitrev(j)).  The points must lie in the prime-order subgroup (not validated); the
    all-zero point is infinity.  A host source is a bytes-like object, a device source
    (src_on_device) a device pointer.  Without dst the result comes back as bytes; with
    dst=<device pointer> (which may be the source) it is written there, ordered on
    `stream`, and None is returned."""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if not 0 <= log_n <= 24:
        raise ValueError("log_n must be in [0, 24]")
    if batch < 0:
        raise ValueError("batch must be >= 0")
    nbytes = (batch << log_n) * POINT_BYTES[group]
    src = points if src_on_device else _fr_host(points, nbytes, "points")
    flags = (NTT_INVERSE if inverse else 0) | (POLY_BITREV if bitrev else 0)
    if dst is not None:
        check(lib().msm_points_ntt(group, device, dst, src, log_n, batch, flags, int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * max(nbytes, 1))()
    check(lib().msm_points_ntt(group, device, out, src, log_n, batch, flags, int(bool(src_on_device)), 0, stream))
    return bytes(out)[:nbytes]


def ntt_model(data, log_n, *, inverse=False, bitrev=False):
    """One transform of 2^log_n blst_fr elements by the schedule of ps_ntt run on the host
    with Fr elements in place of points (msm_points_ntt_model; log_n <= 16), under the
    MSM_POINTS_NTT_SLICE / MSM_POINTS_NTT_CHUNK set now."""
    if not 0 <= log_n <= 16:
        raise ValueError("log_n must be in [0, 16]")
    nbytes = FR_BYTES << log_n
    src = _fr_host(data, nbytes, "elements")
    out = (ctypes.c_uint8 * nbytes)()
    check(lib().msm_points_ntt_model(log_n, (NTT_INVERSE if inverse else 0) | (POLY_BITREV if bitrev else 0), out, src))
    return bytes(out)


class KZGContext:
    """KZG over one Lagrange-form SRS (msm_kzg_*): srs is 2^log_n blst_p1_affine points
    L_i = [l_i(tau)]G1 in the order of the polynomials (natural, or bit-reversed with
    bitrev), tau_g2 the 192 bytes of [tau]G2 (blst_p2_affine, host).  Polynomials are
    2^log_n blst_fr values each; points and values blst_fr; commitments and proofs
    blst_p1_affine (all zero: infinity)."""

    def __init__(self, log_n, srs, tau_g2, *, bitrev=False, srs_on_device=False, device=0, stream=None):
        if not 0 <= log_n <= 20:
            raise ValueError("log_n must be in [0, 20]")
        self.log_n, self.n, self.device, self.bitrev = log_n, 1 << log_n, device, bool(bitrev)
        src = srs if srs_on_device else _fr_host(srs, self.n * POINT_BYTES[1], "SRS points")
        tau = _fr_host(tau_g2, POINT_BYTES[2], "tau_g2")
        self._h = ctypes.c_void_p()
        check(lib().msm_kzg_ctx_create(ctypes.byref(self._h), device, log_n, src, int(bool(srs_on_device)), tau,
                                       POLY_BITREV if bitrev else 0, stream))

    @classmethod
    def from_monomial(cls, log_n, srs_monomial, tau_g2, *, bitrev=False, srs_on_device=False, device=0, stream=None):
        """The context over the SRS given in monomial form: 2^log_n blst_p1_affine points
        [tau^i]G1, i in natural order (msm_kzg_ctx_create_monomial: their inverse ps_ntt on
        the device, bit-reversed with bitrev)."""
        if not 0 <= log_n <= 20:
            raise ValueError("log_n must be in [0, 20]")
        self = cls.__new__(cls)
        self._h = None
        self.log_n, self.n, self.device, self.bitrev = log_n, 1 << log_n, device, bool(bitrev)
        src = srs_monomial if srs_on_device else _fr_host(srs_monomial, self.n * POINT_BYTES[1], "SRS points")
        tau = _fr_host(tau_g2, POINT_BYTES[2], "tau_g2")
        h = ctypes.c_void_p()
        check(lib().msm_kzg_ctx_create_monomial(ctypes.byref(h), device, log_n, src, int(bool(srs_on_device)), tau,
                                                POLY_BITREV if bitrev else 0, stream))
        self._h = h
        return self

    def commit(self, polys, count=1, *, src_on_device=False, dst=None, stream=None):
        """count commitments [f_j(tau)]G1 (bytes; with dst=<device pointer> written there, None returned)"""
        src = polys if src_on_device else _fr_host(polys, count * self.n * FR_BYTES, "polynomial values")
        if dst is not None:
            check(lib().msm_kzg_commit(self._h, dst, src, count, int(bool(src_on_device)), 1, stream))
            return None
        out = (ctypes.c_uint8 * max(count * POINT_BYTES[1], 1))()
        check(lib().msm_kzg_commit(self._h, out, src, count, int(bool(src_on_device)), 0, stream))
        return bytes(out)[:count * POINT_BYTES[1]]

    def open(self, polys, z, count=1, *, src_on_device=False, proofs_dst=None, y_dst=None, stream=None):
        """(proofs, y): proofs[j] = [((f_j - y_j) / (X - z_j))(tau)]G1 and y[j] = f_j(z[j]); with
        proofs_dst and y_dst (device pointers, both) written there and None returned"""
        if src_on_device:
            sp, sz_ = polys, z
        else:
            sp = _fr_host(polys, count * self.n * FR_BYTES, "polynomial values")
            sz_ = _fr_host(z, count * FR_BYTES, "points")
        if (proofs_dst is None) != (y_dst is None):
            raise ValueError("proofs_dst and y_dst go together")
        if proofs_dst is not None:
            check(lib().msm_kzg_open(self._h, proofs_dst, y_dst, sp, sz_, count, int(bool(src_on_device)), 1, stream))
            return None
        pr = (ctypes.c_uint8 * max(count * POINT_BYTES[1], 1))()
        y = (ctypes.c_uint8 * max(count * FR_BYTES, 1))()
        check(lib().msm_kzg_open(self._h, pr, y, sp, sz_, count, int(bool(src_on_device)), 0, stream))
        return bytes(pr)[:count * POINT_BYTES[1]], bytes(y)[:count * FR_BYTES]

    def verify(self, commitments, z, y, proofs, count, *, weights=None, nbits=64, stride=None, batch_offsets=None,
               src_on_device=False, stream=None):
        """The verdict bytes (1: holds).  Without weights one per tuple (C_j, z_j, y_j, pi_j).
        With weights (host bytes: count little-endian strings of `stride` >= (nbits + 7) / 8
        bytes, the low nbits bits used) one per batch of batch_offsets (None: one batch of
        all tuples): the weighted sums of the batch in one pairing check."""
        if src_on_device:
            pc, pz, py, ppi = commitments, z, y, proofs
        else:
            pc = _sig_points("commitments", commitments, count, POINT_BYTES[1], False)
            ppi = _sig_points("proofs", proofs, count, POINT_BYTES[1], False)
            pz = _sig_points("points", z, count, FR_BYTES, False)
            py = _sig_points("values", y, count, FR_BYTES, False)
        wb, bo, nb, nchk = None, None, 0, count
        nbits = int(nbits)
        if weights is not None:
            if nbits < 0 or nbits > 256:
                raise ValueError("nbits must be in 0 .. 256")
            nby = (nbits + 7) // 8
            stride = nby if stride is None else int(stride)
            if stride < nby:
                raise ValueError("stride shorter than (nbits + 7) / 8")
            wb = _sig_points("weights", weights, 1, max((count - 1) * stride + nby, 0), False) if count else None
            nchk = 1
            if batch_offsets is not None:
                offs = _check_offsets("batch_offsets", batch_offsets)
                if offs[-1] > count:
                    raise ValueError(f"batch_offsets ends at {offs[-1]} with {count} tuples")
                bo, nb = (ctypes.c_size_t * len(offs))(*offs), len(offs) - 1
                nchk = nb
        if count == 0:
            return b""
        ok = (ctypes.c_uint8 * max(nchk, 1))()
        nfail = ctypes.c_size_t(0)
        check(lib().msm_kzg_verify(self._h, ok, ctypes.byref(nfail), pc, pz, py, ppi, count, wb, nbits, stride or 0, bo,
                                   nb, int(bool(src_on_device)), stream))
        out = bytes(ok[:nchk])
        assert nfail.value == sum(1 for v in out if not v)
        return out

    def close(self):
        if self._h:
            lib().msm_kzg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _segments(group, points, scalars, offsets, nbits, stride, src_on_device, dst, device, stream):
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    offs = [int(v) for v in offsets]
    if not offs:
        raise ValueError("offsets must hold nsegments + 1 values")
    if offs[0] < 0 or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError("offsets must be non-negative and non-decreasing")
    k = len(offs) - 1
    n = offs[-1] if k else 0  # no segment: nothing is read
    nb = 0
    if scalars is not None:
        if not 0 <= nbits <= 256:
            raise ValueError("nbits must be in [0, 256]")
        nb = (nbits + 7) // 8
        if stride < nb:
            raise ValueError(f"stride {stride} shorter than the {nb} bytes of a {nbits}-bit scalar")
    else:
        nbits = stride = 0
    if src_on_device:
        pts, sc = points, scalars
    else:
        pts = _buf(points)
        have = len(pts) if hasattr(pts, "__len__") else ctypes.sizeof(pts)
        if have < POINT_BYTES[group] * n:
            raise ValueError(f"{have} bytes of points given, {POINT_BYTES[group] * n} needed")
        sc = None
        if scalars is not None:
            sc = _buf(scalars)
            have = len(sc) if hasattr(sc, "__len__") else ctypes.sizeof(sc)
            need = (n - 1) * stride + nb if n else 0
            if have < need:
                raise ValueError(f"{have} bytes of scalars given, {need} needed")
    o = (ctypes.c_size_t * (k + 1))(*offs)
    if dst is not None:
        check(lib().msm_points_msm_segments(group, device, dst, pts, sc, o, k, nbits, stride, 0,
                                            int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * (POINT_BYTES[group] * k))()
    check(lib().msm_points_msm_segments(group, device, out, pts, sc, o, k, nbits, stride, 0, int(bool(src_on_device)),
                                        0, stream))
    return bytes(out)


def ps_msm_segments(group, points, scalars, offsets, *, nbits=255, stride=32, src_on_device=False, dst=None, device=0,
                    stream=None):
    """k MSMs over k point sets in one call (msm_points_msm_segments): out[j] = the sum
    over offsets[j] <= i < offsets[j + 1] of [k_i] P_i, as k affine points (infinity, and
    every empty segment, is the all-zero point).  offsets: any sequence of k + 1
    non-decreasing ints; offsets[-1] points and scalars are read, those below offsets[0]
    ignored.  k_i, nbits and stride as in ps_mult; the result is exact for every point
    of the curve.  Host sources are bytes-like objects, device sources (src_on_device,
    both) device pointers.  With dst=<device pointer> the points are written there,
    ordered on `stream`, and None is returned."""
    if scalars is None:
        raise ValueError("scalars missing (ps_sum_segments sums without scalars)")
    return _segments(group, points, scalars, offsets, nbits, stride, src_on_device, dst, device, stream)


def ps_sum_segments(group, points, offsets, *, src_on_device=False, dst=None, device=0, stream=None):
    """k sums over k point sets in one call (msm_points_msm_segments without scalars):
    out[j] = the sum of the points offsets[j] <= i < offsets[j + 1]; a loop over
    blst_p{1,2}s_add with the results made affine.  Arguments as ps_msm_segments."""
    return _segments(group, points, None, offsets, 0, 0, src_on_device, dst, device, stream)


def segments_plan(offsets, piece):
    """The pieces (start, count, segment) that a piece length cuts offsets into
    (msm_segments_plan; host only)."""
    offs = [int(v) for v in offsets]
    k = len(offs) - 1
    o = (ctypes.c_size_t * (k + 1))(*offs)
    npieces = ctypes.c_size_t(0)
    check(lib().msm_segments_plan(o, k, piece, ctypes.byref(npieces), None, None, None, 0))
    n = npieces.value
    st, ct, sg = ((ctypes.c_size_t * max(n, 1))() for _ in range(3))
    check(lib().msm_segments_plan(o, k, piece, ctypes.byref(npieces), st, ct, sg, n))
    return [(st[i], ct[i], sg[i]) for i in range(n)]


def _h2c_messages(group, msgs, offsets, msg_len, aug, aug_len, src_on_device, n=None):
    """(n, msgs pointer or buffer, offsets array or None, msg_len, aug pointer / buffer or None, aug_len)
    of a hash-to-curve call, checked before any device work"""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if isinstance(msgs, (list, tuple)):
        if offsets is not None or msg_len is not None or src_on_device:
            raise ValueError("a list of messages brings its own offsets and lives in host memory")
        parts = [bytes(p) for p in msgs]
        offsets = [0]
        for p in parts:
            offsets.append(offsets[-1] + len(p))
        msgs = b"".join(parts)
    if (offsets is None) == (msg_len is None):
        raise ValueError("give exactly one of offsets and msg_len")
    if aug_len < 0:
        raise ValueError("aug_len must be >= 0")
    if offsets is not None:
        offs = [int(v) for v in offsets]
        if not offs:
            raise ValueError("offsets must hold n + 1 values")
        if offs[0] < 0 or any(b < a for a, b in zip(offs, offs[1:])):
            raise ValueError("offsets must be non-negative and non-decreasing")
        n, need, ml = len(offs) - 1, offs[-1], 0
        o = (ctypes.c_size_t * len(offs))(*offs)
    else:
        ml = int(msg_len)
        if ml < 0:
            raise ValueError("msg_len must be >= 0")
        if src_on_device:
            if n is None or n < 0:
                raise ValueError("fixed-length messages in device memory need n")
        else:
            have = len(msgs)
            if n is None:
                if ml == 0 or have % ml:
                    raise ValueError(f"{have} bytes of messages are no multiple of msg_len {ml}")
                n = have // ml
            elif n < 0:
                raise ValueError("n must be >= 0")
        need, o = n * ml, None
    if aug is None:
        aug_len = 0
    if src_on_device:
        return n, msgs, o, ml, aug, aug_len
    src = _buf(msgs) if need else None
    if need:
        have = len(src) if hasattr(src, "__len__") else ctypes.sizeof(src)
        if have < need:
            raise ValueError(f"{have} bytes of messages given, {need} needed")
    a = None
    if aug is not None and aug_len:
        a = _buf(aug)
        have = len(a) if hasattr(a, "__len__") else ctypes.sizeof(a)
        if have < n * aug_len:
            raise ValueError(f"{have} bytes of aug given, {n * aug_len} needed")
    return n, src, o, ml, a, aug_len


def ps_map_to_curve(group, u, n, *, count=2, src_on_device=False, dst=None, device=0, stream=None):
    """n points from n * count field elements (msm_points_map): out[i] is the affine form
    of blst_map_to_g{1,2}(u[i count], u[i count + 1] if count == 2), infinity the all-zero
    point.  u: elements in blst's Montgomery layout, 48 G bytes each, canonical; nothing
    is validated.  A host source is a bytes-like object, a device source (src_on_device)
    a device pointer.  With dst=<device pointer> the points are written there, ordered on
    `stream`, and None is returned."""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if n < 0:
        raise ValueError("n must be >= 0")
    if count not in (1, 2):
        raise ValueError("count must be 1 or 2")
    if src_on_device:
        src = u
    else:
        src = _buf(u)
        have = len(src) if hasattr(src, "__len__") else ctypes.sizeof(src)
        if have < n * count * 48 * group:
            raise ValueError(f"{have} bytes of field elements given, {n * count * 48 * group} needed")
    if dst is not None:
        check(lib().msm_points_map(group, device, dst, src, n, count, int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * (POINT_BYTES[group] * n))()
    check(lib().msm_points_map(group, device, out, src, n, count, int(bool(src_on_device)), 0, stream))
    return bytes(out)


def ps_hash_to_field(group, msgs, *, dst_tag, count=2, offsets=None, msg_len=None, n=None, aug=None, aug_len=0,
                     src_on_device=False, dst=None, device=0, stream=None):
    """count field elements per message (msm_hash_to_field): RFC 9380 hash_to_field over
    expand_message_xmd with SHA-256, in blst's Montgomery layout (48 G bytes each), what
    the reference's hash_to_field yields.  Messages, offsets, aug and dst_tag as in
    ps_hash_to_curve."""
    if count not in (1, 2):
        raise ValueError("count must be 1 or 2")
    n, src, o, ml, a, al = _h2c_messages(group, msgs, offsets, msg_len, aug, aug_len, src_on_device, n)
    tag = bytes(dst_tag)
    if dst is not None:
        check(lib().msm_hash_to_field(group, device, dst, src, o, ml, a, al, n, tag, len(tag), count,
                                      int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * (48 * group * count * n))()
    check(lib().msm_hash_to_field(group, device, out, src, o, ml, a, al, n, tag, len(tag), count,
                                  int(bool(src_on_device)), 0, stream))
    return bytes(out)


def ps_hash_to_curve(group, msgs, *, dst_tag, offsets=None, msg_len=None, n=None, aug=None, aug_len=0, encode=False,
                     src_on_device=False, dst=None, device=0, stream=None):
    """One point per message (msm_points_hash): the affine form of blst_hash_to_g{1,2}, or
    with encode of blst_encode_to_g{1,2}, under the domain separation tag dst_tag (host
    bytes, any length).  msgs: a list of bytes objects, or one bytes-like object (device
    pointer with src_on_device) cut by offsets (n + 1 non-decreasing ints) or into
    msg_len-byte messages (n of them; n may be left out for host memory).  aug: n * aug_len bytes in the memory space of msgs, slice i
    hashed in front of message i.  With dst=<device pointer> the points are written
    there, ordered on `stream`, and None is returned."""
    n, src, o, ml, a, al = _h2c_messages(group, msgs, offsets, msg_len, aug, aug_len, src_on_device, n)
    tag = bytes(dst_tag)
    flags = H2C_ENCODE if encode else 0
    if dst is not None:
        check(lib().msm_points_hash(group, device, dst, src, o, ml, a, al, n, tag, len(tag), flags,
                                    int(bool(src_on_device)), 1, stream))
        return None
    out = (ctypes.c_uint8 * (POINT_BYTES[group] * n))()
    check(lib().msm_points_hash(group, device, out, src, o, ml, a, al, n, tag, len(tag), flags,
                                int(bool(src_on_device)), 0, stream))
    return bytes(out)


def h2c_dst_prime(dst_tag):
    """DST_prime = DST || I2OSP(len, 1) after the oversize rule (msm_h2c_dst_prime; host only)."""
    tag = bytes(dst_tag)
    out = (ctypes.c_uint8 * 256)()
    n = ctypes.c_size_t(0)
    check(lib().msm_h2c_dst_prime(out, ctypes.byref(n), tag, len(tag)))
    return bytes(out[:n.value])


_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def fp12_one():
    """blst_fp12_one(): the 576 bytes of the GT value one (2^384 mod p in blst's limbs, then zeros)."""
    return ((1 << 384) % _P).to_bytes(48, "little") + bytes(FP12_BYTES - 48)


def _pair_sources(p, q, n, src_on_device):
    if src_on_device:
        return p, q
    bufs = []
    for data, size, what in ((p, POINT_BYTES[1], "p"), (q, POINT_BYTES[2], "q")):
        b = _buf(data)
        have = len(b) if hasattr(b, "__len__") else ctypes.sizeof(b)
        if have < size * n:
            raise ValueError(f"{have} bytes of {what} given, {size * n} needed")
        bufs.append(b)
    return bufs


def _pairing(p, q, offs, k, n, final_exp, check_only, src_on_device, dst, device, stream):
    pb, qb = _pair_sources(p, q, n, src_on_device)
    o = (ctypes.c_size_t * (k + 1))(*offs) if offs is not None else None
    flags = 0 if final_exp else PAIRING_MILLER_ONLY
    sd = int(bool(src_on_device))
    if check_only:
        verdict = (ctypes.c_uint8 * max(k, 1))()
        check(lib().msm_pairing_segments(device, None, verdict, None, pb, qb, o, k, flags, sd, 0, stream))
        return bytes(verdict[:k])
    if dst is not None:
        check(lib().msm_pairing_segments(device, dst, None, None, pb, qb, o, k, flags, sd, 1, stream))
        return None
    out = (ctypes.c_uint8 * (FP12_BYTES * k))()
    check(lib().msm_pairing_segments(device, out, None, None, pb, qb, o, k, flags, sd, 0, stream))
    return bytes(out)


def _pair_offsets(offsets):
    offs = [int(v) for v in offsets]
    if not offs:
        raise ValueError("offsets must hold nsegments + 1 values")
    if offs[0] < 0 or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError("offsets must be non-negative and non-decreasing")
    k = len(offs) - 1
    return offs, k, (offs[-1] if k else 0)


def ps_pairing(p, q, n, *, final_exp=True, src_on_device=False, dst=None, device=0, stream=None):
    """n pairings e(P_i, Q_i) in one call (msm_pairing_segments without offsets): n GT
    values of FP12_BYTES bytes, byte for byte blst_final_exp(blst_miller_loop(Q_i, P_i)).
    p: n G1 affine points (96 B), q: n G2 affine points (192 B); a pair with infinity on
    either side gives one.  final_exp=False returns the Miller values (equal to the
    reference's only after the final exponentiation).  Host sources are bytes-like
    objects, device sources (src_on_device, both) device pointers.  With dst=<device
    pointer> the values are written there, ordered on `stream`, and None is returned."""
    if n < 0:
        raise ValueError("n must be >= 0")
    return _pairing(p, q, None, n, n, final_exp, False, src_on_device, dst, device, stream)


def ps_pairing_segments(p, q, offsets, *, final_exp=True, src_on_device=False, dst=None, device=0, stream=None):
    """k pairing products in one call (msm_pairing_segments): out[j] = the final
    exponentiation of the product of the Miller values of the pairs offsets[j] <= i <
    offsets[j + 1] (one for an empty segment).  offsets as in ps_msm_segments; the other
    arguments as in ps_pairing."""
    offs, k, n = _pair_offsets(offsets)
    return _pairing(p, q, offs, k, n, final_exp, False, src_on_device, dst, device, stream)


def ps_pairing_check(p, q, offsets, *, src_on_device=False, device=0, stream=None):
    """The verdicts of k pairing products (msm_pairing_segments with dst NULL): bytes of
    k values, 1 where the product of segment j is one."""
    offs, k, n = _pair_offsets(offsets)
    return _pairing(p, q, offs, k, n, True, True, src_on_device, None, device, stream)


def ps_final_exp(f, n, *, src_on_device=False, dst=None, device=0, stream=None):
    """n final exponentiations (msm_fp12_final_exp): blst_final_exp of n canonical
    blst_fp12 values (a zero value gives zero, as the reference does).  Arguments as
    in ps_pairing."""
    if n < 0:
        raise ValueError("n must be >= 0")
    if src_on_device:
        src = f
    else:
        src = _buf(f)
        have = len(src) if hasattr(src, "__len__") else ctypes.sizeof(src)
        if have < FP12_BYTES * n:
            raise ValueError(f"{have} bytes of Fp12 values given, {FP12_BYTES * n} needed")
    sd = int(bool(src_on_device))
    if dst is not None:
        check(lib().msm_fp12_final_exp(device, dst, None, None, src, n, sd, 1, stream))
        return None
    out = (ctypes.c_uint8 * (FP12_BYTES * n))()
    check(lib().msm_fp12_final_exp(device, out, None, None, src, n, sd, 0, stream))
    return bytes(out)


def _sig_points(what, data, n, size, on_device):
    if on_device:
        return data
    if n == 0:
        return None
    b = _buf(data)
    have = len(b) if hasattr(b, "__len__") else ctypes.sizeof(b)
    if have < n * size:
        raise ValueError(f"{have} bytes of {what} given, {n * size} needed")
    return b


def _check_offsets(what, offsets):
    offs = [int(v) for v in offsets]
    if not offs:
        raise ValueError(f"{what} must hold nchecks + 1 values")
    if offs[0] < 0 or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError(f"{what} must be non-negative and non-decreasing")
    return offs


def _sigs(mode, scheme, pks, sigs, msgs, check_offsets, pk_offsets, scalars, nbits, stride, dst_tag, offsets, msg_len,
          n, aug, aug_len, encode, encoded, src_on_device, device, stream):
    if scheme not in (SIG_MIN_PK, SIG_MIN_SIG):
        raise ValueError("scheme must be SIG_MIN_PK (1) or SIG_MIN_SIG (2)")
    kg, sg = scheme, 3 - scheme
    nmsg, src, o, ml, a, al = _h2c_messages(sg, msgs, offsets, msg_len, aug, aug_len, src_on_device, n)
    ksz = (48 if encoded else 96) * kg
    ssz = (48 if encoded else 96) * sg
    if mode == 0:
        k, co, nsig = nmsg, None, nmsg
        if pk_offsets is not None:
            po = _check_offsets("pk_offsets", pk_offsets)
            if len(po) != k + 1:
                raise ValueError(f"pk_offsets holds {len(po)} values for {k} messages")
            nkeys, pko = po[-1], (ctypes.c_size_t * len(po))(*po)
        else:
            nkeys, pko = k, None
    else:
        co = _check_offsets("check_offsets", check_offsets)
        k = len(co) - 1
        if co[-1] > nmsg:
            raise ValueError(f"check_offsets ends at {co[-1]} with {nmsg} messages")
        nkeys, nsig, pko = co[-1], (k if mode == 1 else co[-1]), None
    kb = _sig_points("public keys", pks, nkeys, ksz, src_on_device)
    sb = _sig_points("signatures", sigs, nsig, ssz, src_on_device)
    flags = (H2C_ENCODE if encode else 0) | (SIG_ENCODED if encoded else 0)
    tag = bytes(dst_tag)
    sd = int(bool(src_on_device))
    status = (ctypes.c_uint8 * max(k, 1))()
    nfail = ctypes.c_size_t(0)
    L = lib()
    if mode == 0:
        check(L.msm_sigs_verify(scheme, device, status, ctypes.byref(nfail), kb, pko, sb, src, o, ml, a, al, k, tag,
                                len(tag), flags, sd, stream))
    else:
        cof = (ctypes.c_size_t * len(co))(*co)
        if mode == 1:
            check(L.msm_sigs_aggregate_verify(scheme, device, status, ctypes.byref(nfail), kb, sb, src, o, ml, a, al,
                                              cof, k, tag, len(tag), flags, sd, stream))
        else:
            nbits = int(nbits)
            if nbits < 0 or nbits > 256:
                raise ValueError("nbits must be in 0 .. 256")
            nb = (nbits + 7) // 8
            stride = nb if stride is None else int(stride)
            if scalars is not None and stride < nb:
                raise ValueError("stride shorter than (nbits + 7) / 8")
            wb = None
            if scalars is not None:
                wb = scalars if src_on_device else _sig_points("scalars", scalars, 1, max((co[-1] - 1) * stride + nb, 0),
                                                               False) if co[-1] else None
            check(L.msm_sigs_batch_verify(scheme, device, status, ctypes.byref(nfail), kb, sb, wb, nbits, stride, src,
                                          o, ml, a, al, cof, k, tag, len(tag), flags, sd, stream))
    out = bytes(status[:k])
    assert nfail.value == sum(1 for v in out if v)
    return out


def ps_verify(scheme, pks, sigs, msgs, *, dst_tag, pk_offsets=None, offsets=None, msg_len=None, n=None, aug=None,
              aug_len=0, encode=False, encoded=False, src_on_device=False, device=0, stream=None):
    """One status byte per signature (msm_sigs_verify): check i verifies signature i over
    message i under the sum of the keys pk_offsets[i] .. pk_offsets[i + 1] (without
    pk_offsets: key i), as blst_core_verify_pk_in_g{1,2} does.  scheme: SIG_MIN_PK (keys in
    G1) or SIG_MIN_SIG (keys in G2).  Status: 0 success, 1 bad encoding, 2 not on curve,
    3 not in group, 5 verify fail, 6 public key is infinity.  pks / sigs: blst affine
    points, or with encoded compressed ZCash entries; messages, offsets, aug, dst_tag and
    encode as in ps_hash_to_curve; everything in host memory, or with src_on_device
    device pointers."""
    return _sigs(0, scheme, pks, sigs, msgs, None, pk_offsets, None, 0, None, dst_tag, offsets, msg_len, n, aug,
                 aug_len, encode, encoded, src_on_device, device, stream)


def ps_aggregate_verify(scheme, pks, sigs, msgs, check_offsets, *, dst_tag, offsets=None, msg_len=None, n=None,
                        aug=None, aug_len=0, encode=False, encoded=False, src_on_device=False, device=0, stream=None):
    """One status byte per aggregate signature (msm_sigs_aggregate_verify): check j verifies
    signature j over the (key, message) tuples check_offsets[j] .. check_offsets[j + 1], the
    reference's blst_pairing_chk_n_aggr_pk_in_g{1,2} / commit / finalverify sequence.  The
    other arguments and the statuses as in ps_verify."""
    return _sigs(1, scheme, pks, sigs, msgs, check_offsets, None, None, 0, None, dst_tag, offsets, msg_len, n, aug,
                 aug_len, encode, encoded, src_on_device, device, stream)


def ps_batch_verify(scheme, pks, sigs, msgs, check_offsets, *, dst_tag, scalars=None, nbits=64, stride=None,
                    offsets=None, msg_len=None, n=None, aug=None, aug_len=0, encode=False, encoded=False,
                    src_on_device=False, device=0, stream=None):
    """One status byte per batch (msm_sigs_batch_verify): check j verifies the (key, message,
    signature, scalar) tuples check_offsets[j] .. check_offsets[j + 1] with one final
    exponentiation, the reference's blst_pairing_chk_n_mul_n_aggr_pk_in_g{1,2} / commit /
    finalverify sequence.  scalars: the weights, nbits bits each, stride (default (nbits +
    7) // 8) bytes apart, little-endian; they must be unpredictable to the signers.
    scalars=None or nbits=0: the unweighted form.  The other arguments and the statuses as
    in ps_verify."""
    return _sigs(2, scheme, pks, sigs, msgs, check_offsets, None, scalars, nbits, stride, dst_tag, offsets, msg_len, n,
                 aug, aug_len, encode, encoded, src_on_device, device, stream)


def ps_in_group(group, points, n, *, src_on_device=False, device=0, stream=None):
    """n bytes, 1 where affine point i lies in the prime-order subgroup (msm_points_in_group:
    blst_p{1,2}_affine_in_g{1,2}; infinity passes).  The points are not modified."""
    if group not in POINT_BYTES:
        raise ValueError("group must be 1 or 2")
    if n < 0:
        raise ValueError("n must be >= 0")
    src = _sig_points("points", points, n, POINT_BYTES[group], src_on_device)
    out = (ctypes.c_uint8 * max(n, 1))()
    check(lib().msm_points_in_group(group, device, out, src, n, int(bool(src_on_device)), stream))
    return bytes(out[:n])


def sigs_plan(mode, check_offsets, pk_offsets, nchecks, c0, chunk):
    """The chunk of checks that starts at c0 (msm_sigs_plan; host only): a dict with c1,
    rows, keys, sigs, ent (list of (check, source)), pair_off, key_off, sig_off."""
    co = (ctypes.c_size_t * len(check_offsets))(*check_offsets) if check_offsets is not None else None
    po = (ctypes.c_size_t * len(pk_offsets))(*pk_offsets) if pk_offsets is not None else None
    c1 = ctypes.c_size_t(0)
    counts = (ctypes.c_size_t * 4)()
    check(lib().msm_sigs_plan(mode, co, po, nchecks, c0, chunk, ctypes.byref(c1), counts, None, None, None, None, None, 0))
    nent, nc = counts[3], c1.value - c0
    cap = max(nent, nc + 1)
    ec, es = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)()
    pf, kf, sf = (ctypes.c_size_t * cap)(), (ctypes.c_size_t * cap)(), (ctypes.c_size_t * cap)()
    check(lib().msm_sigs_plan(mode, co, po, nchecks, c0, chunk, ctypes.byref(c1), counts, ec, es, pf, kf, sf, cap))
    return {"c1": c1.value, "rows": counts[0], "keys": counts[1], "sigs": counts[2],
            "ent": [(ec[i], es[i]) for i in range(nent)], "pair_off": list(pf[:nc + 1]),
            "key_off": list(kf[:nc + 1]) if mode == 0 and po is not None else [],
            "sig_off": list(sf[:nc + 1]) if mode == 2 else []}


def sigs_reduce(mode, check_offsets, pk_offsets, c0, c1, sig_codes, key_codes, late, is_one):
    """The statuses of the checks [c0, c1) from the screen's codes (msm_sigs_reduce; host only)."""
    co = (ctypes.c_size_t * len(check_offsets))(*check_offsets) if check_offsets is not None else None
    po = (ctypes.c_size_t * len(pk_offsets))(*pk_offsets) if pk_offsets is not None else None
    out = (ctypes.c_uint8 * max(c1 - c0, 1))()
    check(lib().msm_sigs_reduce(mode, co, po, c0, c1, bytes(sig_codes) + b"\0", bytes(key_codes) + b"\0",
                                bytes(late) if late is not None else None, bytes(is_one) + b"\0", out))
    return bytes(out[:c1 - c0])


def to_affine_levels(n):
    """Product levels of the batch inversion above n points (msm_to_affine_levels)."""
    return lib().msm_to_affine_levels(n)


def _mult(group, points, scalars, n, nbits):
    """blst calling convention with the {ptr, NULL} flat shortcut (multi_scalar.c:393-416)."""
    pts = _buf(points)
    sc = _buf(scalars)
    pp = (ctypes.c_void_p * 2)(ctypes.cast(pts, ctypes.c_void_p), None)
    sp = (ctypes.c_void_p * 2)(ctypes.cast(sc, ctypes.c_void_p), None)
    ret = (ctypes.c_uint8 * JAC_BYTES[group])()
    getattr(lib(), f"blst_p{group}s_mult_pippenger")(ret, pp, n, sp, nbits, None)
    return bytes(ret)


def p1s_mult_pippenger(points, scalars, n, nbits=255):
    """G1 MSM; scalars packed with stride (nbits+7)//8.  Returns blst_p1 bytes (Jacobian)."""
    return _mult(1, points, scalars, n, nbits)


def p2s_mult_pippenger(points, scalars, n, nbits=255):
    return _mult(2, points, scalars, n, nbits)


def ps_add(group, points, n):
    """Sum of n affine points (blst_p1s_add / blst_p2s_add, ref bulk_addition.c:145-164), flat array."""
    pts = _buf(points)
    pp = (ctypes.c_void_p * 2)(ctypes.cast(pts, ctypes.c_void_p), None)
    ret = (ctypes.c_uint8 * JAC_BYTES[group])()
    getattr(lib(), f"blst_p{group}s_add")(ret, pp, n)
    return bytes(ret)


class MSMContext:
    """Device-resident points on one GPU; repeated MSMs over new scalars.

    window_bits: Pippenger window c (bucket count 2^(c-1) per window); 0 = 16.
    """

    def __init__(self, group=1, device=0, window_bits=0):
        self.group = group
        self._ctx = ctypes.c_void_p()
        check(lib().msm_ctx_create(ctypes.byref(self._ctx), group, device, window_bits))
        self.n = 0
        self.first_bad = None  # index of the entry the last set_points_encoded rejected

    def set_points(self, points, n, on_device=False, stream=None):
        ptr = points if on_device else _buf(points)
        check(lib().msm_ctx_set_points(self._ctx, ptr, n, int(bool(on_device)), stream))
        self.n = n

    def set_points_encoded(self, data, n, compressed=True, check_group=True, on_device=False, stream=None):
        """Points from n ZCash-encoded entries (see ps_decode), decoded on the GPU into a
        buffer the context owns.  Any rejected entry raises MsmError (self.first_bad holds
        its index) and the context keeps its previous points."""
        src, enc = _encoded(self.group, data, n, compressed, on_device)
        bad = ctypes.c_size_t(0)
        self.first_bad = None
        rc = lib().msm_ctx_set_points_encoded(self._ctx, src, n, enc, DECODE_CHECK_GROUP if check_group else 0,
                                              int(bool(on_device)), ctypes.byref(bad), stream)
        if rc != 0 and "rejected" in lib().msm_last_error().decode(errors="replace"):
            self.first_bad = bad.value
        check(rc)
        self.n = n

    def mult(self, scalars, nbits=255, stride=32, on_device=False, stream=None):
        ret = (ctypes.c_uint8 * JAC_BYTES[self.group])()
        ptr = scalars if on_device else _buf(scalars)
        check(lib().msm_ctx_mult(self._ctx, ret, ptr, stride, nbits, int(bool(on_device)), stream))
        return bytes(ret)

    def mult_batch(self, scalars, count, nbits=255, stride=32, set_stride=None, on_device=False, stream=None):
        """`count` pipelined MSMs (scalar set k at k * set_stride bytes); returns a
        list of Jacobian byte strings, equal to `count` mult() calls."""
        if set_stride is None:
            set_stride = self.n * stride
        nb = JAC_BYTES[self.group]
        rets = (ctypes.c_uint8 * (nb * count))()
        ptr = scalars if on_device else _buf(scalars)
        check(lib().msm_ctx_mult_batch(self._ctx, rets, ptr, stride, set_stride, nbits, count, int(bool(on_device)),
                                       stream))
        raw = bytes(rets)
        return [raw[k * nb:(k + 1) * nb] for k in range(count)]

    def set_profiling(self, on=True):
        check(lib().msm_ctx_set_profiling(self._ctx, int(on)))

    def phase_times(self):
        out = (ctypes.c_float * 6)()
        check(lib().msm_ctx_phase_times(self._ctx, out))
        return dict(zip(("digits", "sort", "accumulate", "reduce", "finalize", "total"), list(out)))

    def close(self):
        if self._ctx:
            lib().msm_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
