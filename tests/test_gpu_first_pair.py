"""GPU parity of a bucket's first add (ec.hpp xyzz_madd with acc_affine set:
the accumulation kernels skip the four products by ZZ1 = ZZZ1 = 1 when the
second entry meets the bucket xyzz_from_aff just started).

Plain Pippenger contexts, c = 8, n <= 512, G1 and G2 (lane pairs), against the
CPU oracle.  Scalars below 2^7 have the single window-0 digit v (bucket v,
positive), so the scalar of a row chooses its bucket and the number of rows
with one scalar chooses the bucket's entry count; the scalar 256 - v puts the
row into bucket v negated (digit v - 256 with a carry: one more, positive,
entry in bucket 1 of window 1).  Rows are repeated the way
test_equal_points_doubling_branch builds its own where equal or opposite
entries are wanted.
"""
import ctypes

import pytest

import oracle_ffi as of

pytestmark = pytest.mark.gpu

C = 8


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


def _sc(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def _check(m, group, rows, values, oracle_skip=()):
    """rows: list of affine rows (bytes), values: their scalars; the oracle sums
    the rows not listed in oracle_skip (affine infinity rows)"""
    n = len(rows)
    assert n == len(values) and n <= 512
    ctx = m.MSMContext(group, 0, C)
    ctx.set_points(b"".join(rows), n)
    got = m.compress(group, ctx.mult(_sc(values), 255)).hex()
    ctx.close()
    keep = [i for i in range(n) if i not in oracle_skip]
    pts = b"".join(rows[i] for i in keep)
    sc = _sc(values[i] for i in keep)
    cp = (ctypes.c_uint8 * len(pts)).from_buffer_copy(pts)
    cs = (ctypes.c_uint8 * len(sc)).from_buffer_copy(sc)
    assert got == of.compress(group, of.msm(group, cp, cs, len(keep), 255, "naive"))


def _rows(m, group, n):
    raw = bytes(m.fixed_points(group, n))
    w = 96 * group
    return [raw[w * i:w * (i + 1)] for i in range(n)]


@pytest.mark.parametrize("group", [1, 2])
def test_two_entries_in_every_bucket(m, group):
    """(a) 127 buckets of exactly two distinct entries: every madd is a first add"""
    rows = _rows(m, group, 254)
    _check(m, group, rows, [1 + i // 2 for i in range(254)])


@pytest.mark.parametrize("group", [1, 2])
def test_one_two_three_entries_mixed(m, group):
    """(b) buckets of one, two and three entries side by side: the waves of the
    count-ordered schedule hold lanes whose second iteration has the flag, lanes
    that are done and lanes that go on to a generic third add"""
    values = []
    for v in range(1, 128):
        values += [v] * (1 + v % 3)
    rows = _rows(m, group, len(values))
    _check(m, group, rows, values)


@pytest.mark.parametrize("group", [1, 2])
def test_first_two_entries_equal(m, group):
    """(c) the first two entries of a bucket are the same point: PP == 0 from the
    affine state, the doubling branch; a third, distinct entry follows in half
    of the buckets"""
    base = _rows(m, group, 96)
    rows, values = [], []
    for v in range(1, 33):
        rows += [base[v], base[v]]
        values += [v, v]
        if v % 2:
            rows.append(base[32 + v])
            values.append(v)
    _check(m, group, rows, values)


@pytest.mark.parametrize("group", [1, 2])
def test_first_two_entries_opposite_then_two_more(m, group):
    """(d) +P then -P (scalar 256 - v) leave infinity, the third entry starts
    the bucket again and the fourth is a first add once more: the flag is set
    twice in one bucket.  Both orders of the opposite pair."""
    base = _rows(m, group, 200)
    rows, values = [], []
    for v in range(2, 42):
        a, b = (v, 256 - v) if v % 2 else (256 - v, v)
        rows += [base[v], base[v], base[50 + v], base[100 + v]]
        values += [a, b, v, v]
    _check(m, group, rows, values)


@pytest.mark.parametrize("group", [1, 2])
def test_affine_infinity_row_first(m, group):
    """(e) the first row of the bucket is all-zero (affine infinity, skipped):
    the bucket starts at its second row and the third is its first add"""
    base = _rows(m, group, 130)
    w = 96 * group
    rows, values, skip = [], [], []
    for v in range(1, 41):
        skip.append(len(rows))
        rows += [bytes(w), base[v], base[64 + v]]
        values += [v, v, v]
    _check(m, group, rows, values, oracle_skip=skip)


@pytest.mark.parametrize("group", [1, 2])
def test_sign_flipped_entries(m, group):
    """(f) the first entry negated (xyzz_from_aff's reduced -Y), the second
    negated (the first add's reduced -Y2), both, and neither"""
    base = _rows(m, group, 256)
    rows, values = [], []
    for v in range(2, 66):
        f1, f2 = (v >> 0) & 1, (v >> 1) & 1
        rows += [base[v], base[128 + v]]
        values += [256 - v if f1 else v, 256 - v if f2 else v]
        if v % 5 == 0:  # and a generic third add after it
            rows.append(base[70 + v])
            values.append(256 - v if v % 10 else v)
    _check(m, group, rows, values)


def test_ches_n10_golden(m, golden):
    """CHES n = 2^10 (k_accumulate over the table rows) against its golden key"""
    n = 1024
    want = [c for c in golden("msm_g1.json")["cases"]
            if c["n"] == n and c["seed"] == 1 and c["case"] == "rand" and c["nbits"] == 255][0]["compressed"]
    ctx = m.CHESContext(1, 0, n_exp=10)
    ctx.build_table(m.fixed_points(1, n), n)
    got = m.compress(1, ctx.mult(m.gen_scalars(n, 1))).hex()
    ctx.close()
    assert got == want
