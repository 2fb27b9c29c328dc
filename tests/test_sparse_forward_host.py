"""The checkers of tests/test_gpu_sparse_forward.py, checked themselves - no device.

On the small planted graph (tile 256): a sequential numpy-fp32 sum passes ``check_equal`` on exact inputs and
``check_gamma`` on real ones; every way a tiled kernel loses an edge - dropped at the first, the last or the ragged last
position of a tile, dropped inside the hub, doubled while another is dropped, credited across a tile boundary, a
non-zero in an empty row - fails ``check_equal``, and fails ``check_gamma`` too unless the row has more than 1,000 edges
(there gamma_L A exceeds one term, which is why the exact inputs exist).  The planted graph has the positions it
claims, the plan's class table is the restated rule's, and ``assert_exact`` holds for every graph the GPU file uses."""
import numpy as np
import pytest

import _spmm_fwd_ref as R
from oracle import kgat_oracle as orc

TE, C, D = 256, (4, 8, 16), 8


@pytest.fixture(scope="module")
def G():
    g = R.planted_csr(TE, C, 0, 1)
    g["row_of"] = np.repeat(np.arange(g["n"]), g["deg"])
    g["Xe"], we = R.exact_inputs(g["n"], g["e"], D, 2)
    rng = np.random.default_rng(3)
    g["Xr"] = rng.standard_normal((g["n"], D)).astype(np.float32)
    wr = rng.random(g["e"]).astype(np.float32)
    for k, X, w in (("e", g["Xe"], we), ("r", g["Xr"], wr)):
        g["w" + k] = w[g["eid"]]                   # CSR order
        g["ref" + k] = orc.spmm_u_mul_e_sum(g["n"], g["src"], g["dst"], X, w)
        g["A" + k] = orc.spmm_u_mul_e_sum(g["n"], g["src"], g["dst"], np.abs(X), np.abs(w))
    return g


def _both(G, rows_of_pos=None, mult=None):
    rp = G["row_of"] if rows_of_pos is None else rows_of_pos
    return (R.seq_sum32(G["n"], rp, G["col"], G["Xe"], G["we"], mult),
            R.seq_sum32(G["n"], rp, G["col"], G["Xr"], G["wr"], mult))


def test_sequential_fp32_sum_passes_both_checks(G):
    R.assert_exact(G["Ae"], G["Xe"])
    exact, real = _both(G)
    R.check_equal(exact, G["refe"], "sequential fp32, exact inputs")
    R.check_gamma(real, G["refr"], G["Ar"], G["deg"], 0, "sequential fp32, real inputs")
    R.check_equal(exact * G["Xe"], G["refe"] * G["Xe"], "mul_self, exact inputs")
    R.check_gamma(real * G["Xr"], G["refr"] * G["Xr"], G["Ar"] * np.abs(G["Xr"]), G["deg"], 1, "mul_self, real inputs")
    ones = np.ones((G["n"], D), np.float32)
    cnt = R.seq_sum32(G["n"], G["row_of"], G["col"], ones, np.ones(G["e"], np.float32))
    assert np.array_equal(cnt, np.broadcast_to(G["deg"][:, None].astype(np.float32), cnt.shape))
    mean = R.mean_exact(cnt, G["deg"])
    assert np.array_equal(mean, (G["deg"] > 0).astype(np.float32)[:, None] * ones)


def _mutations(G):
    """name -> (rows credited per position, multiplicity per position, the mutated row)."""
    e, row_of, ip = G["e"], G["row_of"], G["indptr"]
    hub = G["rows"]["hub"][0]
    out = {}

    def drop(name, p):
        m = np.ones(e, np.float32)
        m[p] = 0
        out[name] = (row_of, m, int(row_of[p]))
    drop("dropped: first position of a tile", TE)
    drop("dropped: last position of a tile", TE - 1)
    drop("dropped: last ragged position", e - 1)
    drop("dropped: inside the hub", int(ip[hub]) + 5 * TE + 17)
    # doubled + dropped in one row (the one-tile row): a pair of positions whose terms differ in the exact inputs
    r = G["rows"]["one_tile"][0]
    p = int(ip[r]) + 10
    terms = G["we"][:, None] * G["Xe"][G["col"]]
    q = next(q for q in range(int(ip[r]) + 11, int(ip[r + 1])) if np.any(terms[q] != terms[p]))
    m = np.ones(e, np.float32)
    m[p], m[q] = 2, 0
    out["doubled, another of the row dropped"] = (row_of, m, r)
    moved = row_of.copy()
    assert row_of[TE - 1] + 1 == row_of[TE]
    moved[TE - 1] = row_of[TE]                    # the last edge of tile 0 credited to the row tile 1 starts with
    out["credited to the neighbouring row across a tile boundary"] = (moved, None, int(row_of[TE - 1]))
    return out


MUTATIONS = ["dropped: first position of a tile", "dropped: last position of a tile", "dropped: last ragged position",
             "dropped: inside the hub", "doubled, another of the row dropped",
             "credited to the neighbouring row across a tile boundary"]


@pytest.mark.parametrize("name", MUTATIONS)
def test_every_lost_edge_is_caught(G, name):
    muts = _mutations(G)
    assert sorted(muts) == sorted(MUTATIONS)
    rows_of_pos, mult, row = muts[name]
    exact, real = _both(G, rows_of_pos, mult)
    with pytest.raises(AssertionError):
        R.check_equal(exact, G["refe"], name)
    if G["deg"][row] <= 1000:
        with pytest.raises(AssertionError):
            R.check_gamma(real, G["refr"], G["Ar"], G["deg"], 0, name)
    else:
        assert name == "dropped: inside the hub"


def test_nonzero_in_an_empty_row_is_caught(G):
    exact, real = _both(G)
    assert G["deg"][0] == 0
    exact[0, 3], real[0, 3] = 0.25, 1e-30
    with pytest.raises(AssertionError):
        R.check_equal(exact, G["refe"], "non-zero in an empty row")
    with pytest.raises(AssertionError):
        R.check_gamma(real, G["refr"], G["Ar"], G["deg"], 0, "non-zero in an empty row")


@pytest.mark.parametrize("TE_,e_min", [(64, 0), (128, 0), (256, 0), (512, 0), (256, 262_145), (512, 1_048_577)])
def test_planted_graph_is_what_it_claims(TE_, e_min):
    Cs = R.GRAPH_SPECS[(TE_, e_min)]
    g = R.planted_csr(TE_, Cs, e_min, 11)
    n, src, dst, deg = R.planted_graph(TE_, Cs, e_min, 11)
    assert n == g["n"] and np.array_equal(src, g["src"]) and np.array_equal(deg, g["deg"])
    ip, rows, e = g["indptr"], g["rows"], g["e"]
    assert e == len(src) == len(dst) and np.array_equal(np.bincount(dst, minlength=n), deg)
    # CSR order is the stable sort by destination, and it is not the edge-id order
    eid = np.argsort(dst, kind="stable")
    assert np.array_equal(eid, g["eid"]) and np.array_equal(src[eid], g["col"])
    assert not np.array_equal(eid, np.arange(e))
    assert deg[0] == 0 and ip[3] == TE_ and deg[2] == 3                   # a row that ends exactly on a boundary
    r = rows["one_tile"][0]
    assert ip[r] == TE_ and ip[r + 1] == 2 * TE_                          # a row that is exactly one tile
    h = rows["hub"][0]
    assert ip[h] % TE_ == 0 and (ip[h + 1] - 1) // TE_ - ip[h] // TE_ >= R.K_LONG_CHAIN
    lo, hi = rows["ones"]
    assert hi - lo == 2 * TE_ + 7 and np.all(deg[lo:hi] == 1)
    lo, hi = rows["empty"]
    assert hi - lo == 50 and np.all(deg[lo:hi] == 0)
    for c in np.atleast_1d(Cs):
        for d in (c - 1, c, c + 1):
            assert np.sum(deg[slice(*rows["runs"])] == d) >= 6
    for d in R.SMALL_DEGREES:
        assert np.sum(deg[slice(*rows["small"])] == d) == 6
    c0 = rows["chain"][0]
    assert deg[c0] == 3 * TE_ + 1 and 3 <= (ip[c0 + 1] - 1) // TE_ - ip[c0] // TE_ < R.K_LONG_CHAIN
    assert deg[c0 + 1] == deg[c0 + 2] == 0
    a = rows["aligned"][0]
    assert ip[a] % TE_ == 0 and deg[a] == 2 * TE_ and deg[a - 1] > 0
    assert e > e_min and e % 4 != 0 and e % TE_ != 0
    assert list(deg[-4:-2]) == [0, deg[-3]] and deg[-3] >= 5 and deg[-2] == deg[-1] == 0
    assert np.array_equal(g["col"][:8], np.repeat(np.arange(n), deg)[:8])  # self-loops
    pair = dst.astype(np.int64) * n + src
    assert len(np.unique(pair)) < e                                       # parallel edges


def test_class_table_is_the_restated_rule():
    for Dw, (short, half, full) in R.CLASS_TABLE.items():
        assert R.tile_rule(Dw, 1) == ("short", R.tile_rule(Dw, 1)[1], short[0])
        assert R.tile_rule(Dw, short[1])[::2] == ("short", short[0])
        nxt = R.tile_rule(Dw, short[1] + 1)
        if half is None:
            assert nxt[::2] == ("full", full)
        else:
            assert nxt[::2] == ("half", half[0]) and R.tile_rule(Dw, half[1])[::2] == ("half", half[0])
            assert R.tile_rule(Dw, half[1] + 1)[::2] == ("full", full)
        for cls_e in (1, short[1] + 1, 9_000_000):
            _, c, te = R.tile_rule(Dw, cls_e)
            assert te == c * ((128 if Dw <= 32 else 256) // (Dw // 4))


def test_assert_exact_holds_for_every_gpu_graph():
    """4 max A < 2^24 on the float64 reference of every graph the GPU file builds (four columns of the exact inputs:
    the columns are identically distributed), and from the degree sequence alone for any draw: A <= 6 deg, times
    |X[v]| <= 3 for the mul_self forms.  The GPU cases assert it again on the reference they compare with."""
    for (TE_, e_min), Cs in R.GRAPH_SPECS.items():
        g = R.planted_csr(TE_, Cs, e_min, R.graph_seed(TE_, e_min))
        X, w = R.exact_inputs(g["n"], g["e"], 4, 5)
        A = orc.spmm_u_mul_e_sum_sparse(g["n"], g["src"], g["dst"], np.abs(X), w)
        top = R.assert_exact(A, X)
        worst = 4.0 * 6.0 * 3.0 * float(g["deg"].max())
        print("(TE %d, e_min %d): n %d e %d  4 max A = %d, worst case for any draw %d" % (TE_, e_min, g["n"], g["e"], top, worst))
        assert top <= worst < 2 ** 24
    with pytest.raises(AssertionError):
        R.assert_exact(np.full((2, 2), 2.0 ** 22))
