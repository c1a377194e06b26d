"""Inputs and a plain-integer model of the bulk signature verification
(tests/test_sigs_host.py, tests/test_gpu_sigs.py, tests/golden/make_sigs_golden.py).

A *call* is one invocation of ps_verify / ps_aggregate_verify / ps_batch_verify:
  mode      0 verify, 1 aggregate, 2 batch
  scheme    1 min-pk (keys in G1), 2 min-sig (keys in G2)
  variant   "hash", "encode" (encode-to-curve), "aug" (a 7-byte aug per message)
  keys      list of items, sigs list of items, msgs list of bytes (one per row)
  o         the check offsets (aggregate, batch) or None; pk_off the key sets or None
  weights   list of ints or None, nbits
An item is a point ((x, y) or None for infinity) or ("raw", <encoded bytes>): an
entry that exists only in the encoded form of a table.

Signed tuples come from one pool per (scheme, variant): seeded 96-bit secret
keys sk_i, pk_i = [sk_i] g, sig_i = [sk_i] H(m_i).  The model restates the
sequence of the header: per tuple the signature (uncompress code, infinity
skipped, 3 outside the group), then each key (uncompress code, 6 infinite, 3
outside the group), for key sets 6 when the sum is infinite, and last the pairing
product (pairing_inputs.py) -- 0 when it is one, else 5; no tuples: 5.
"""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enc_inputs as ei  # noqa: E402
import h2c_inputs as hi  # noqa: E402
import mult_inputs as mi  # noqa: E402
import pairing_inputs as pi  # noqa: E402
from jac_inputs import fnv  # noqa: E402,F401

MIN_PK, MIN_SIG = 1, 2
VERIFY, AGGREGATE, BATCH = 0, 1, 2
AUG_LEN = 7
N_POOL = 80
MSG_LENGTHS = [0, 1, 55, 56, 64, 200]
VARIANT_POOL = {"hash": N_POOL, "encode": 12, "aug": 12}


def tag(scheme):
    """the DST of the scheme's hashes (they lie in the group of the signatures)"""
    return hi.DST[3 - scheme]


def message(i):
    if i < len(MSG_LENGTHS):
        return hi._bytes(MSG_LENGTHS[i], 17 + i)
    return b"sig-msg-%04d" % i + hi._bytes(i % 29, i)


def aug_of(i):
    return hi._bytes(AUG_LEN, 300 + i)


def neg(g, pt):
    return hi.neg_pt(g, pt)


def add(g, p, q):
    return hi.add_pt(g, p, q)


@functools.lru_cache(maxsize=None)
def pool(scheme, variant="hash"):
    """[(sk, pk, msg, aug, H, sig)] of the signed tuples"""
    n = VARIANT_POOL[variant]
    kg, sg = scheme, 3 - scheme
    sks = [k % (1 << 96) | 1 for k in mi.gen_scalars(n, 0x5160 + 16 * scheme + len(variant))]
    out = []
    for i, sk in enumerate(sks):
        m = message(i)
        a = aug_of(i) if variant == "aug" else b""
        h = hi.hash_to_curve(sg, m, tag(scheme), a, encode=variant == "encode")
        out.append((sk, mi.smul(kg, ei.GEN[kg], sk), m, a, h, mi.smul(sg, h, sk)))
    return out


@functools.lru_cache(maxsize=None)
def off_group(g, i):
    x = ei.OFF_GROUP[g][i]
    y = ei.f_sqrt(g, ei.curve_rhs(g, x))
    assert y is not None
    return (x, y)


def raw_bad_encoding(g):
    return ("raw", bytes([0x20]) + bytes(ei.ENC[g] - 1))  # no compression bit


def raw_off_curve(g, i=0):
    return ("raw", ei.with_flags(ei.be_bytes(g, ei.OFF_CURVE[g][i]), 0x80))


# ------------------------------------------------------------------ the calls ----
def _call(mode, scheme, variant, keys, sigs, rows, o=None, pk_off=None, weights=None, nbits=0):
    pl = pool(scheme, variant)
    return dict(mode=mode, scheme=scheme, variant=variant, keys=keys, sigs=sigs, rows=list(rows),
                msgs=[pl[i][2] for i in rows], augs=[pl[i][3] for i in rows], o=o, pk_off=pk_off, weights=weights,
                nbits=nbits)


def individual(scheme, variant="hash", encoded=False):
    """about 40 checks (45 encoded): (key, signature, message) each"""
    kg, sg = scheme, 3 - scheme
    pl = pool(scheme, variant)
    n = len(pl) if variant != "hash" else 28
    keys, sigs, rows = [], [], []

    def case(key, sig, row):
        keys.append(key), sigs.append(sig), rows.append(row)

    for i in range(n):  # valid: the message lengths first
        case(pl[i][1], pl[i][5], i)
    case(pl[0][1], pl[1][5], 0)                      # forged: the signature of another message
    case(pl[3][1], pl[2][5], 2)                      # a wrong key
    case(None, pl[2][5], 2)                          # an infinite key: 6
    case(pl[2][1], None, 2)                          # an infinite signature: 5
    case(off_group(kg, 0), pl[4][5], 4)              # key outside its group: 3
    case(pl[4][1], off_group(sg, 1), 4)              # signature outside its group: 3
    case(off_group(kg, 2), off_group(sg, 3), 5)      # both: the signature's code
    case(None, off_group(sg, 4), 5)                  # infinite key, bad signature: 3, not 6
    case(None, None, 5)                              # both infinite: 6
    case(pl[6][1], neg(sg, pl[6][5]), 6)             # the negated signature
    case(neg(kg, pl[7][1]), pl[7][5], 7)             # the negated key
    case(off_group(kg, 4), None, 8)                  # infinite signature, key outside: 3
    if encoded:
        case(raw_bad_encoding(kg), pl[8][5], 8)                  # 1 on the key
        case(raw_off_curve(kg), pl[8][5], 8)                     # 2 on the key
        case(pl[9][1], raw_bad_encoding(sg), 9)                  # 1 on the signature
        case(pl[9][1], raw_off_curve(sg, 1), 9)                  # 2 on the signature
        case(raw_bad_encoding(kg), raw_off_curve(sg, 2), 10)     # both: the signature's 2
    return _call(VERIFY, scheme, variant, keys, sigs, rows)


def key_sets(scheme):
    """sets of 0, 1, 2 and 7 keys; P and -P; a bad key and an infinite key in the middle"""
    kg, sg = scheme, 3 - scheme
    pl = pool(scheme)
    keys, sigs, rows, off = [], [], [], [0]

    def check(members, row, extra=None):
        """signed by the members' keys over message `row`; extra: (position, key) put in place"""
        h, sk = pl[row][4], sum(pl[i][0] for i in members)
        ks = [pl[i][1] for i in members]
        if extra:
            ks[extra[0]] = extra[1]
        keys.extend(ks)
        sigs.append(mi.smul(sg, h, sk % ei.R) if members else pl[row][5])
        rows.append(row)
        off.append(off[-1] + len(ks))

    check([], 10)
    check([11], 11)
    check([12, 13], 12)
    check(list(range(14, 21)), 14)
    keys.extend([pl[21][1], neg(kg, pl[21][1])])  # the sum is infinite: 6
    sigs.append(pl[21][5]), rows.append(21), off.append(off[-1] + 2)
    check([22, 23, 24], 22, extra=(1, off_group(kg, 1)))  # 3
    check([25, 26, 27], 25, extra=(1, None))              # 6
    check([28, 29], 28)
    sigs[-1] = pl[28][5]                                   # the signature of one of the two keys alone: 5
    return _call(VERIFY, scheme, "hash", keys, sigs, rows, pk_off=off)


def _aggregate_sig(scheme, members):
    pl = pool(scheme)
    s = None
    for i in members:
        s = add(3 - scheme, s, pl[i][5])
    return s


AGG_LENGTHS = [0, 1, 2, 5, 17]


def aggregate(scheme):
    """lengths 0, 1, 2, 5 and 17, then checks of 5 with an error at the first, a middle and the last tuple"""
    kg, sg = scheme, 3 - scheme
    pl = pool(scheme)
    keys, sigs, rows, o = [], [], [], [0]
    nxt = [30]

    def check(length, edit=None, sig=Ellipsis):
        members = list(range(nxt[0], nxt[0] + length))
        nxt[0] += length
        ks = [pl[i][1] for i in members]
        if edit:
            ks[edit[0]] = edit[1]
        keys.extend(ks), rows.extend(members)
        sigs.append(_aggregate_sig(scheme, members) if sig is Ellipsis else sig)
        o.append(o[-1] + length)

    for ln in AGG_LENGTHS:
        check(ln)
    check(5, edit=(0, off_group(kg, 0)))   # 3
    check(5, edit=(2, None))               # 6
    check(5, edit=(4, off_group(kg, 3)))   # 3
    check(2, sig=pl[0][5])                 # another signature: 5
    check(2, sig=None)                     # an infinite signature: 5
    check(2, edit=(1, None), sig=off_group(sg, 0))  # the signature's 3 before the key's 6
    assert nxt[0] <= N_POOL
    return _call(AGGREGATE, scheme, "hash", keys, sigs, rows, o=o)


def _weights(n, nbits, seed):
    return [(k % (1 << nbits)) | 1 for k in mi.gen_scalars(n, seed)]


def batch(scheme, kind="w64"):
    """kind w64: checks of 1, 2, 9 and 33 tuples, one with a forged signature, the cancelling
    pair, an empty check, a signature outside its group, an infinite key; w255: 255-bit
    weights; w0: nbits == 0"""
    kg, sg = scheme, 3 - scheme
    pl = pool(scheme)
    keys, sigs, rows, o = [], [], [], [0]

    def check(members, edit_sig=None, edit_key=None):
        ks, ss = [pl[i][1] for i in members], [pl[i][5] for i in members]
        if edit_sig:
            ss[edit_sig[0]] = edit_sig[1]
        if edit_key:
            ks[edit_key[0]] = edit_key[1]
        keys.extend(ks), sigs.extend(ss), rows.extend(members)
        o.append(o[-1] + len(members))

    if kind == "w64":
        check([0])
        check([1, 2])
        check(list(range(3, 12)))
        check(list(range(12, 45)))
        check(list(range(45, 54)), edit_sig=(4, pl[0][5]))         # one forged signature: 5
        check([54, 54], edit_sig=(1, neg(sg, pl[54][5])))           # (pk, m, sig), (pk, m, -sig)
        check([])                                                   # no tuples: 5
        check([55, 56, 57], edit_sig=(1, off_group(sg, 2)))         # 3
        check([58, 59, 60], edit_key=(2, None))                     # 6
        check([61, 62], edit_sig=(0, None))                         # an infinite signature is skipped: 5
        nbits = 64
    elif kind == "w255":
        check([0, 1])
        check(list(range(2, 11)))
        check([11, 12], edit_sig=(1, pl[0][5]))
        nbits = 255
    else:
        check([0])
        check([1, 2])
        check(list(range(3, 12)))
        check([12, 13], edit_sig=(0, pl[13][5]))
        nbits = 0
    w = _weights(len(rows), nbits, 0xba7c4 + nbits) if nbits else None
    if kind == "w64":  # the cancelling pair has equal weights
        w[o[5] + 1] = w[o[5]]
    return _call(BATCH, scheme, "hash", keys, sigs, rows, o=o, weights=w, nbits=nbits)


TABLES = {
    "individual": lambda s: individual(s),
    "individual_encoded": lambda s: individual(s, encoded=True),
    "individual_encode": lambda s: individual(s, "encode"),
    "individual_aug": lambda s: individual(s, "aug"),
    "key_sets": key_sets,
    "aggregate": aggregate,
    "batch_w64": lambda s: batch(s, "w64"),
    "batch_w255": lambda s: batch(s, "w255"),
    "batch_w0": lambda s: batch(s, "w0"),
}
ENCODED_TOO = ("individual_encoded", "key_sets", "aggregate", "batch_w64")  # tables also run in encoded form


@functools.lru_cache(maxsize=None)
def table(name, scheme):
    return TABLES[name](scheme)


def nchecks(call):
    return len(call["rows"]) if call["mode"] == VERIFY else len(call["o"]) - 1


# ------------------------------------------------------------------ the bytes ----
def item_bytes(g, item, encoded):
    if isinstance(item, tuple) and len(item) == 2 and item[0] == "raw":
        assert encoded, "a raw entry exists only in the encoded form"
        return item[1]
    return ei.encode_point(g, item, True) if encoded else ei.affine_bytes(g, item)


def call_bytes(call, encoded=False):
    """the arrays the library takes: keys, sigs, the messages joined and their offsets, aug, scalars"""
    kg, sg = call["scheme"], 3 - call["scheme"]
    nb = (call["nbits"] + 7) // 8
    mo = [0]
    for m in call["msgs"]:
        mo.append(mo[-1] + len(m))
    return dict(keys=b"".join(item_bytes(kg, k, encoded) for k in call["keys"]),
                sigs=b"".join(item_bytes(sg, s, encoded) for s in call["sigs"]),
                msgs=b"".join(call["msgs"]), msg_off=mo,
                aug=b"".join(call["augs"]) if call["variant"] == "aug" else None,
                scalars=b"".join(w.to_bytes(nb, "little") for w in call["weights"]) if call["weights"] else None)


def input_hash(call, encoded=False):
    b = call_bytes(call, encoded)
    return fnv(b["keys"] + b["sigs"] + b["msgs"] + (b["aug"] or b"") + (b["scalars"] or b"") +
               repr((b["msg_off"], call["o"], call["pk_off"], call["nbits"])).encode())


def run(m, call, encoded=False, **kw):
    """the call through the library's Python interface: the status bytes"""
    b = call_bytes(call, encoded)
    common = dict(dst_tag=tag(call["scheme"]), offsets=b["msg_off"], encode=call["variant"] == "encode",
                  encoded=encoded, aug=b["aug"], aug_len=AUG_LEN if b["aug"] else 0, **kw)
    if call["mode"] == VERIFY:
        return m.ps_verify(call["scheme"], b["keys"], b["sigs"], b["msgs"], pk_offsets=call["pk_off"], **common)
    if call["mode"] == AGGREGATE:
        return m.ps_aggregate_verify(call["scheme"], b["keys"], b["sigs"], b["msgs"], call["o"], **common)
    return m.ps_batch_verify(call["scheme"], b["keys"], b["sigs"], b["msgs"], call["o"], scalars=b["scalars"],
                             nbits=call["nbits"], **common)


# ------------------------------------------------------------------ the model ----
def _point_code(g, item, is_key):
    """(code, point): the steps one point goes through"""
    if isinstance(item, tuple) and len(item) == 2 and item[0] == "raw":
        st, pt = ei._uncompress(g, item[1])
        if st:
            return st, None
        item = pt
    if item is None:
        return (6 if is_key else 0), None
    if not ei.in_group(g, ei.affine_bytes(g, item)):
        return 3, None
    return 0, item


def model_status(call, j):
    """the status of check j, by the sequence of the header and the pairing model"""
    scheme, mode = call["scheme"], call["mode"]
    kg, sg = scheme, 3 - scheme
    pl = pool(scheme, call["variant"])
    if mode == VERIFY:
        k0, k1 = (call["pk_off"][j], call["pk_off"][j + 1]) if call["pk_off"] else (j, j + 1)
        tuples = [(j, list(range(k0, k1)), j)]  # (signature index or None, keys, row)
    elif mode == AGGREGATE:
        tuples = [(j if t == call["o"][j] else None, [t], t) for t in range(call["o"][j], call["o"][j + 1])]
    else:
        tuples = [(t, [t], t) for t in range(call["o"][j], call["o"][j + 1])]
    if not tuples:
        return 5
    S, pairs = None, []
    for si, ks, row in tuples:
        w = call["weights"][row] if call["weights"] else 1
        if si is not None:
            code, s = _point_code(sg, call["sigs"][si], False)
            if code:
                return code
            S = add(sg, S, mi.smul(sg, s, w) if s is not None else None)
        ksum = None
        for t in ks:
            code, k = _point_code(kg, call["keys"][t], True)
            if code:
                return code
            ksum = add(kg, ksum, k)
        if ksum is None:
            return 6
        h = pl[call["rows"][row]][4]
        if kg == 1:
            pairs.append((mi.smul(1, ksum, w), h))
        else:
            pairs.append((mi.smul(1, h, w), ksum))
    pairs.append((pi.NEG_G1, S) if kg == 1 else (S, (pi.G2[0], pi.f2_neg(pi.G2[1]))))
    return 0 if pi.f12_is_one(pi.pairing_product(pairs)) else 5
