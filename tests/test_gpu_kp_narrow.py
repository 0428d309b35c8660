"""Stored fp64 tiles at 53 bits per value (csrc/kp_narrow.hpp, DESIGN.md §3.1.2, PLSSVM_MI_OPT_KP_PACK).

A packable tile whose values lie in two adjacent binades is stored as 52 mantissa bits + 1 exponent bit per value
("narrow"), any other packable tile at 7 bytes per value, the rest raw; the form is chosen per tile by the fill and
decoded while the tile is streamed. Every decode is exact, so every result must be BITWISE what the other forms and
the implicit product give: all comparisons here are np.array_equal.

Shapes: d = 20. m = 256 (3 tiles) and m = 384 (6 tiles) have no padded rows, so the form of every tile follows from
the data and the counts are exact; m = 130 and m = 300 have padded rows in the last tile row, whose entries decide
those tiles' form, so only the order narrow <= packed <= tiles is asserted there.
"""
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import datagen

pytestmark = pytest.mark.gpu

D = 20
TILE = 128
DTYPES = {"f64": np.float64, "f32": np.float32}
GAMMA = 1.0      # grouped data: cluster tiles narrow, every tile with spread rows 7-byte
GAMMA_MID = 2.5  # grouped data: narrow, 7-byte and raw tiles in one cache
MARGIN = 1e-6    # every kernel value keeps this relative distance from a power of two


def _tiles(m):
    nb = -(-m // TILE)
    return nb * (nb + 1) // 2


@functools.lru_cache(maxsize=None)
def _blobs(m, dtype, seed=11):
    X, y = datagen.blobs(m + 1, D, seed=seed, dtype=DTYPES[dtype])
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def _grouped(kinds="ABS", seed=2):
    """128 rows per letter, plus the last point (which the system eliminates). A / B: tight clusters (1e-3 around a
    centre) whose centres are exactly 1 apart; S: spread around A's centre, squared radii uniform in [0.3, 3]. With
    gamma = 1: k = exp(-d^2) is within [0.5, 1] inside a cluster, next to e^-1 (inside [0.25, 0.5)) between A and B,
    and between e^-0.3 and e^-3 (five binades) from S to A."""
    rng = np.random.default_rng(seed)
    cA = rng.uniform(-0.5, 0.5, D)
    delta = rng.standard_normal(D)
    delta /= np.linalg.norm(delta)
    rows = []
    for kind in kinds + "S":
        if kind in "AB":
            rows.append((cA if kind == "A" else cA + delta) + 1e-3 * rng.standard_normal((TILE, D)))
        else:
            u = rng.standard_normal((TILE, D))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            rows.append(cA + np.sqrt(rng.uniform(0.3, 3.0, (TILE, 1))) * u)
    m = TILE * len(kinds)
    X = np.concatenate(rows)[: m + 1].copy()
    y = np.where(rng.uniform(size=m + 1) < 0.5, -1.0, 1.0)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _form(k, diag):
    """The form of one tile of positive kernel values, and its binade span, as kp_narrow_desc classifies it. Every
    value must stay MARGIN away from a power of two, so that neither the device's exp nor the centred data can move it
    into another binade. The diagonal of a diagonal tile is exp(-gamma * 0) up to the rounding of n_i + n_i - 2 g_ii:
    1.0 or just below, and the form must be the same either way."""
    assert k.min() > 1e-290
    forms = []
    for one in ((1.0, np.nextafter(1.0, 0.0)) if diag else (None,)):
        v = k.copy()
        off = ~np.eye(TILE, dtype=bool) if diag else np.ones_like(v, dtype=bool)
        frac = np.frexp(v[off])[0]  # in [0.5, 1)
        assert (frac - 0.5 >= 0.5 * MARGIN).all() and (1.0 - frac >= MARGIN).all(), "a value too close to a power of two"
        if diag:
            v[~off] = one
        e = np.frexp(v)[1]
        span = int(e.max() - e.min())
        forms.append(("narrow" if span <= 1 else "wide" if span <= 15 else "raw", span))
    assert len({f for f, _ in forms}) == 1, forms
    return forms[0]


@functools.lru_cache(maxsize=None)
def _host_forms(kinds, gamma, first=0):
    """{(I, J): (form, span)} of the lower-triangle tiles of rows [first, first + m), from numpy."""
    X = _grouped(kinds)[0][first:-1]
    nb = X.shape[0] // TILE
    out = {}
    for I in range(nb):
        for J in range(I + 1):
            a, b = X[I * TILE:(I + 1) * TILE], X[J * TILE:(J + 1) * TILE]
            d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
            out[(I, J)] = _form(np.exp(-gamma * d2), I == J)
    return out


def _counts(forms):
    names = [f for f, _ in forms.values()]
    return names.count("narrow"), names.count("narrow") + names.count("wide")


def _vectors(m, dtype, count=3):
    rng = np.random.default_rng(200 + m)
    return [rng.uniform(-1, 2, m).astype(DTYPES[dtype]) for _ in range(count)]


def _svm(kernel, dtype, data, gamma=1.0 / D, coef0=0.5, **kw):
    X, y = data
    p = pm.Parameter(kernel, gamma=gamma, coef0=coef0, real_type=DTYPES[dtype])
    p.data, p.labels = X.astype(DTYPES[dtype], copy=False), y.astype(DTYPES[dtype], copy=False)
    if kernel == "linear":
        kw.setdefault("kp_mode", "pairwise")
    return pm.CSVM(p, **kw)


def _kps(svm, m, dtype="f64"):
    """Three K·p with different p on a fresh setup: with the cache on, the first fills and the others stream."""
    svm.setup_data_on_device()
    svm.generate_q()
    return [svm.run_device_kernel(None, np.zeros(m, DTYPES[dtype]), v, 1.0).copy() for v in _vectors(m, dtype)]


def _data(which, m):
    if which == "blobs":
        return _blobs(m, "f64")
    if which == "BS":  # m = 256: cluster B and the spread rows of "ABS"
        X, y = _grouped("ABS")
        return X[TILE:], y[TILE:]
    return _grouped(which)


@functools.lru_cache(maxsize=None)
def _implicit(which, m, gamma):
    """The implicit product (cache off), computed once per case and shared."""
    with _svm("rbf", "f64", _data(which, m), gamma, kp_cache=False) as svm:
        out = _kps(svm, m)
        info = svm.info()
    assert info["kp_cache_tiles"] == 0 and info["kp_cache_packed_tiles"] == 0 and info["kp_cache_narrow_tiles"] == 0
    for o in out:
        assert np.isfinite(o).all() and np.abs(o).max() > 0
        o.setflags(write=False)
    return tuple(out)


def _assert_all_equal(got, want, tag):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (tag, k, np.abs(g - w).max())


def _ordered(info, m):
    assert info["kp_cache_tiles"] == _tiles(m)
    assert 0 <= info["kp_cache_narrow_tiles"] <= info["kp_cache_packed_tiles"] <= info["kp_cache_tiles"], info


def test_the_grouped_data_is_what_the_counts_assume():
    """On the host: the spans the exact counts below rest on."""
    f = _host_forms("ABS", GAMMA)
    assert f[(0, 0)] == ("narrow", 1) and f[(1, 1)] == ("narrow", 1)  # [0.5, 1) and the diagonal's 1.0
    assert f[(1, 0)] == ("narrow", 0)  # one binade below 0.5
    X = _grouped("ABS")[0]
    k10 = np.exp(-GAMMA * ((X[128:256, None, :] - X[None, :128, :]) ** 2).sum(-1))
    assert 0.25 < k10.min() and k10.max() < 0.5
    k00 = np.exp(-GAMMA * ((X[:128, None, :] - X[None, :128, :]) ** 2).sum(-1))
    assert k00.min() > 0.5
    assert f[(2, 0)][0] == "wide" and 3 <= f[(2, 0)][1] + 1 <= 15  # three or more binades, at most 15 below the top one
    assert _counts(f) == (3, 6)
    mid = _host_forms("ABS", GAMMA_MID)
    assert any(span > 15 for _, span in mid.values())
    assert {form for form, _ in mid.values()} == {"narrow", "wide", "raw"}  # all three forms in one cache
    assert _counts(_host_forms("ABS", GAMMA, TILE)) == (1, 3)  # m = 256: B narrow, the two tiles with spread rows 7-byte


@pytest.mark.parametrize("which,m,gamma", [("BS", 256, GAMMA), ("BS", 256, GAMMA_MID), ("ABS", 384, GAMMA), ("ABS", 384, GAMMA_MID)])
def test_exact_counts_and_bitwise_products(which, m, gamma):
    narrow, packed = _counts(_host_forms("ABS", gamma, TILE if which == "BS" else 0))
    want = _implicit(which, m, gamma)
    with _svm("rbf", "f64", _data(which, m), gamma) as svm:
        auto = _kps(svm, m)
        info = svm.info()
    assert info["kp_cache_tiles"] == _tiles(m)
    assert info["kp_cache_bytes"] == _tiles(m) * TILE * TILE * 8  # the record stride does not change
    assert info["kp_cache_narrow_tiles"] == narrow, info
    assert info["kp_cache_packed_tiles"] == packed, info
    assert narrow <= packed <= _tiles(m) and narrow > 0
    with _svm("rbf", "f64", _data(which, m), gamma, kp_pack="wide") as svm:
        wide = _kps(svm, m)
        info = svm.info()
    assert info["kp_cache_narrow_tiles"] == 0 and info["kp_cache_packed_tiles"] == packed
    with _svm("rbf", "f64", _data(which, m), gamma, kp_pack=False) as svm:
        raw = _kps(svm, m)
        info = svm.info()
    assert info["kp_cache_narrow_tiles"] == 0 and info["kp_cache_packed_tiles"] == 0 and info["kp_cache_tiles"] == _tiles(m)
    _assert_all_equal(auto, want, ("auto/implicit", m, gamma))
    _assert_all_equal(wide, want, ("wide/implicit", m, gamma))
    _assert_all_equal(raw, want, ("raw/implicit", m, gamma))


@pytest.mark.parametrize("m", [130, 300])
def test_padded_shapes(m):
    want = _implicit("blobs", m, 1.0 / D)
    for pack in (None, "wide", False):
        with _svm("rbf", "f64", _blobs(m, "f64"), **({} if pack is None else {"kp_pack": pack})) as svm:
            got = _kps(svm, m)
            info = svm.info()
        _ordered(info, m)
        if pack is not None:
            assert info["kp_cache_narrow_tiles"] == 0
        _assert_all_equal(got, want, ("padded", m, pack))


def test_no_tile_is_counted_before_the_fill():
    m = 384
    narrow, packed = _counts(_host_forms("ABS", GAMMA_MID))
    with _svm("rbf", "f64", _grouped("ABS"), GAMMA_MID) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        info = svm.info()
        assert info["kp_cache_tiles"] == _tiles(m) and info["kp_cache_packed_tiles"] == 0 and info["kp_cache_narrow_tiles"] == 0
        svm.run_device_kernel(None, np.zeros(m), _vectors(m, "f64", 1)[0], 1.0)
        info = svm.info()
        assert (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]) == (narrow, packed)


def test_kp_multi_on_a_cache_with_all_three_forms():
    m, R = 384, 3
    narrow, packed = _counts(_host_forms("ABS", GAMMA_MID))
    assert 0 < narrow < packed < _tiles(m)
    P = np.stack(_vectors(m, "f64", R))
    with _svm("rbf", "f64", _grouped("ABS"), GAMMA_MID) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        single = [svm.run_device_kernel(None, np.zeros(m), P[c], 1.0).copy() for c in range(R)]  # fills, then streams
        info = svm.info()
        assert (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]) == (narrow, packed)
        assert info["multi_width"] >= R
        multi = svm.run_device_kernel_multi(None, np.zeros((R, m)), P, 1.0)
    _assert_all_equal(single, _implicit("ABS", m, GAMMA_MID), "single")
    _assert_all_equal(list(multi), single, "multi")


def _cg61(pack, m=384):
    X, y = _grouped("ABS")
    with _svm("rbf", "f64", (X, y), GAMMA_MID, **({} if pack is None else {"kp_pack": pack})) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        svm.cg_begin(y[:-1] - y[-1], None, eps=1e-3)
        it, _ = svm.cg_step(61, force=True)
        assert it == 61
        x, trace, _ = svm.cg_result(62)
        info = svm.info()
        return x.copy(), trace.copy(), info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]


def test_cg_across_a_graph_block(monkeypatch):
    """61 forced iterations: the every-50th explicit residual and one captured block of iterations."""
    monkeypatch.delenv("PLSSVM_MI_GRAPH", raising=False)
    x1, t1, narrow1, packed1 = _cg61(None)
    x0, t0, narrow0, packed0 = _cg61(False)
    assert (narrow1, packed1) == _counts(_host_forms("ABS", GAMMA_MID)) and (narrow0, packed0) == (0, 0)
    assert len(t1) == 62 and np.isfinite(t1).all()
    assert np.array_equal(t1, t0), np.abs(t1 - t0).max()
    assert np.array_equal(x1, x0), np.abs(x1 - x0).max()


def test_partial_cache(monkeypatch):
    m = 300
    rec = TILE * TILE * 8
    budget = 4 * rec + rec // 2
    want = _implicit("blobs", m, 1.0 / D)
    monkeypatch.setenv("PLSSVM_MI_MEM_BUDGET", str(budget))
    with _svm("rbf", "f64", _blobs(m, "f64")) as svm:
        got = _kps(svm, m)
        info = svm.info()
    assert info["kp_cache_tiles"] == budget // rec == 4  # the descriptors take nothing from the budget
    assert info["kp_cache_bytes"] == 4 * rec
    assert 0 <= info["kp_cache_narrow_tiles"] <= info["kp_cache_packed_tiles"] <= 4
    _assert_all_equal(got, want, "partial")


def test_partial_cache_of_narrow_tiles(monkeypatch):
    """The first four of the six records of the grouped data: (0,0), (1,0), (1,1) narrow, (2,0) 7-byte; (2,1), (2,2) computed."""
    m = 384
    rec = TILE * TILE * 8
    monkeypatch.setenv("PLSSVM_MI_MEM_BUDGET", str(4 * rec + rec // 2))
    with _svm("rbf", "f64", _grouped("ABS"), GAMMA) as svm:
        got = _kps(svm, m)
        info = svm.info()
    assert info["kp_cache_tiles"] == 4
    assert (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]) == (3, 4)
    _assert_all_equal(got, _implicit("ABS", m, GAMMA), "partial narrow")


def test_a_second_setup_rebuilds_descriptors_and_both_counters():
    m = 384
    v = _vectors(m, "f64", 1)[0]
    counts = {k: _counts(_host_forms(k, GAMMA_MID)) for k in ("ABS", "SAS")}
    assert counts["ABS"] != counts["SAS"] and counts["ABS"][0] != counts["SAS"][0]

    def two_products(svm):
        svm.setup_data_on_device()
        svm.generate_q()
        a = svm.run_device_kernel(None, np.zeros(m), v, 1.0).copy()  # fills
        b = svm.run_device_kernel(None, np.zeros(m), v, 1.0).copy()  # streams
        info = svm.info()
        return a, b, (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"])

    fresh = {}
    for kinds in ("ABS", "SAS"):
        with _svm("rbf", "f64", _grouped(kinds), GAMMA_MID) as svm:
            fresh[kinds] = two_products(svm)
        assert np.array_equal(fresh[kinds][0], fresh[kinds][1])
        assert fresh[kinds][2] == counts[kinds]
    for first, second in (("ABS", "SAS"), ("SAS", "ABS")):
        with _svm("rbf", "f64", _grouped(first), GAMMA_MID) as svm:
            got1 = two_products(svm)
            svm.params.data = _grouped(second)[0]
            got2 = two_products(svm)
        for got, want in ((got1, fresh[first]), (got2, fresh[second])):
            assert got[2] == want[2]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(fresh["ABS"][0], _implicit("ABS", m, GAMMA_MID)[0])


def test_the_environment_switch_and_option_value_2_mean_7_byte_only(monkeypatch):
    m = 384
    narrow, packed = _counts(_host_forms("ABS", GAMMA_MID))
    want = _implicit("ABS", m, GAMMA_MID)
    with _svm("rbf", "f64", _grouped("ABS"), GAMMA_MID, kp_pack="wide") as svm:
        got = _kps(svm, m)
        info = svm.info()
    assert (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]) == (0, packed)
    _assert_all_equal(got, want, "option 2")
    monkeypatch.setenv("PLSSVM_MI_KP_NARROW", "0")
    for pack in (None, True):
        with _svm("rbf", "f64", _grouped("ABS"), GAMMA_MID, **({} if pack is None else {"kp_pack": pack})) as svm:
            got = _kps(svm, m)
            info = svm.info()
        assert (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]) == (0, packed)
        _assert_all_equal(got, want, ("env", pack))
    monkeypatch.setenv("PLSSVM_MI_KP_NARROW", "1")
    with _svm("rbf", "f64", _grouped("ABS"), GAMMA_MID) as svm:
        got = _kps(svm, m)
        info = svm.info()
    assert (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]) == (narrow, packed)
    _assert_all_equal(got, want, "env on")
    monkeypatch.setenv("PLSSVM_MI_KP_PACK", "0")  # keeps its meaning: every record raw
    with _svm("rbf", "f64", _grouped("ABS"), GAMMA_MID) as svm:
        got = _kps(svm, m)
        info = svm.info()
    assert (info["kp_cache_narrow_tiles"], info["kp_cache_packed_tiles"]) == (0, 0)
    _assert_all_equal(got, want, "pack env off")


def test_the_narrow_count_has_its_own_entry_point():
    """plssvm_mi_info keeps its size and its last fields; the count comes from plssvm_mi_get_kp_cache_narrow_tiles, which
    CSVM.info() puts beside the struct's fields. Missing arguments are ERR_ARG, not a write."""
    import ctypes

    from plssvm_sparse_fp22_amd import _abi

    L = _abi.lib()
    assert "kp_cache_narrow_tiles" not in [f[0] for f in _abi.Info._fields_]
    narrow, _ = _counts(_host_forms("ABS", GAMMA_MID))
    with _svm("rbf", "f64", _grouped("ABS"), GAMMA_MID) as svm:
        _kps(svm, 384)
        n = ctypes.c_int64(-7)
        assert L.plssvm_mi_get_kp_cache_narrow_tiles(svm._ctx, ctypes.byref(n)) == 0
        assert n.value == narrow == svm.info()["kp_cache_narrow_tiles"]
        assert L.plssvm_mi_get_kp_cache_narrow_tiles(svm._ctx, None) == -1
        assert L.plssvm_mi_get_kp_cache_narrow_tiles(None, ctypes.byref(n)) == -1
    assert n.value == narrow


def test_a_bad_kp_pack_value_is_refused():
    with pytest.raises(ValueError):
        _svm("rbf", "f64", _blobs(130, "f64"), kp_pack="narrow")


@functools.lru_cache(maxsize=None)
def _signed(m):
    """Zero-mean data: every tile of x_i . x_j, and of its cube, holds negative values, so no tile can be packed."""
    rng = np.random.default_rng(17)
    X = rng.uniform(-1, 1, (m + 1, D))
    y = np.where(rng.uniform(size=m + 1) < 0.5, -1.0, 1.0)
    G = X[:m] @ X[:m].T
    nb = -(-m // TILE)
    for I in range(nb):
        for J in range(I + 1):
            assert G[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE].min() < -1e-3
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@pytest.mark.parametrize("kernel,dtype,m", [("linear", "f64", 300), ("polynomial", "f64", 300), ("rbf", "f32", 384),
                                            ("rbf", "f32", 130)])
def test_other_kernels_and_real_types(kernel, dtype, m):
    if kernel == "rbf":  # fp32 records are never packed, whatever the values
        data, gamma = (_grouped("ABS") if m == 384 else _blobs(m, dtype)), (GAMMA if m == 384 else 1.0 / D)
    else:  # (gamma x.y)^3 and x.y keep the signs
        data, gamma = _signed(m), 1.0 / D
    with _svm(kernel, dtype, data, gamma, coef0=0.0, kp_cache=False) as svm:
        want = _kps(svm, m, dtype)
    with _svm(kernel, dtype, data, gamma, coef0=0.0) as svm:
        got = _kps(svm, m, dtype)
        info = svm.info()
    assert info["kp_cache_tiles"] == _tiles(m)
    assert info["kp_cache_narrow_tiles"] == 0 and info["kp_cache_packed_tiles"] == 0
    _assert_all_equal(got, want, (kernel, dtype, m))
