"""The Rankformer passes where tests/test_gpu_rankformer.py does not reach: the chunk geometry of
the two kernels with poisoned outputs and workspace, every branch of the two hand-written
backwards against fp64 autograd of the plain definition, the layer where the clamp is active, on
cut rows, at d = 193 and stacked twice, a graph without pairs, and the sampler beside a user that
holds every item.

Bounds (none of them measured on the device first).

* Kernels (chunk geometry): as in test_gpu_rankformer.py, every output element within
  2 (deg + d) 2^-24 Σ|terms| of the fp64 value, deg the row's length, Σ|terms| in fp64 from absolute
  values; every element finite although outputs and workspace start as NaN; a row of length 0 is
  exactly +0; two calls into differently poisoned buffers give the same bits.
* Autograd functions: both passes are sums of products, so the fp64 plain definition
  (rankformer_ref.plain_rowpass / plain_wsum: gather, multiply, index_add_) run backward on
  |inputs| and |cotangents| gives Σ|terms| of every gradient element exactly. Each device gradient
  element is within 2 (Dmax + d + 4) 2^-24 Σ|terms| of the fp64 gradient: a gradient element is a sum
  over at most Dmax entries (Dmax the longest row of either orientation) of products that hold a dot
  product of d terms; the + 4 covers the added edge scalars (t_e = g_s + g_sum + <gA, V>) and the sum
  of two passes. A gradient that is None counts as zero; where Σ|terms| is zero the bound is zero, so
  it must equal the fp64 gradient exactly.
* Layers against the second fixture (tests/golden/rankformer_layer_more.npz, recorded from the
  reference layer): the largest absolute error against the reference's fp64 output and gradient is
  at most 4 x the reference's own fp32 error on the same input (recorded in the fixture), the
  yardstick and margin of test_gpu_rankformer.py; two runs give the same bits.
* A graph without pairs: every sum of the layer runs over all m items (or n users), so the forward
  bound is 2 (max(n, m) + d + 4) 2^-24 Σ|terms| with Σ|terms| = Σ_j |Ω_uj| |v_j| / (2 D_u) (items
  alike) from the dense definition in fp64. The fused form evaluates Σ_j (s_uj − α) v_j as x̂_u G − α Σ v_j;
  with unit rows Σ_f |x̂_uf x̂_jf| <= 1 <= |s_uj − α| at α = 2, so its terms are no larger than the
  dense ones. Gradient: g_k = Σ_rf W_rf ∂z_rf/∂x_k; Σ|terms| = Σ_rf |W_rf| |∂z_rf/∂x_k| from the fp64
  Jacobian of the dense definition, same factor.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankformer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
GEOM_DIMS = [1, 65, 193]  # J = 1, 2 and 4 features per lane
QUIET_NAN, OTHER_NAN = 0x7FC00000, -1  # two NaN bit patterns (int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def poisoned(n, bits):
    return torch.full((int(n),), bits, dtype=torch.int32, device="cuda").view(torch.float32)


def check(name, got, exact, mag, count):
    """|got − exact| <= 2 count 2^-24 mag elementwise; prints the largest err/bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == exact.shape, (name, got.shape, exact.shape)
    assert np.isfinite(got).all(), name
    bound = 2.0 * count * U24 * mag
    err = np.abs(got - exact)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if got.size else 0.0
    print(f"{name}: max err/bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (name, ratio)
    return ratio


# ---- chunk geometry, poisoned outputs and workspace --------------------------------------------
def pattern_csr(lens, n_cols, seed):
    rng = np.random.RandomState(seed)
    lens = np.asarray(lens, np.int64)
    cols = [np.sort(rng.choice(n_cols, l, replace=l > n_cols)) for l in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32) if lens.sum() else np.zeros(0, np.int32)
    return rowptr, col, lens


def fresh_workspace(lib, nnz, d, bits):
    """Exactly gdd_rank_ws_bytes(nnz, d) bytes, every word a NaN."""
    nbytes = int(lib.gdd_rank_ws_bytes(nnz, d))
    assert nbytes % 4 == 0
    return poisoned(nbytes // 4, bits).view(torch.uint8), nbytes


def raw_rowpass(rowptr, col, n_cols, Q, K, V, bits):
    """gdd_rank_rowpass through the library, into NaN-filled outputs and workspace."""
    from gdd import _lib
    lib = _lib.device_lib()
    n_rows, nnz, d = rowptr.shape[0] - 1, col.shape[0], Q.shape[1]
    rp, cl, Qd, Kd, Vd = dev(rowptr), dev(col), dev(Q), dev(K), dev(V)
    s, s_sum = poisoned(nnz, bits), poisoned(n_rows, bits)
    SK, SV, A = (poisoned(n_rows * d, bits).view(n_rows, d) for _ in range(3))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws, nbytes = fresh_workspace(lib, nnz, d, bits)
    _lib.check(lib.gdd_rank_rowpass(n_rows, n_cols, nnz, rp.data_ptr(), cl.data_ptr() if nnz else None, d,
                                    Qd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), s.data_ptr() if nnz else None,
                                    s_sum.data_ptr(), SK.data_ptr(), SV.data_ptr(), A.data_ptr(), bad.data_ptr(),
                                    ws.data_ptr(), nbytes, _lib.stream_ptr("cuda")))
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    return {"s": s.cpu().numpy(), "s_sum": s_sum.cpu().numpy(), "SK": SK.cpu().numpy(), "SV": SV.cpu().numpy(),
            "A": A.cpu().numpy()}


def raw_wsum(rowptr, col, n_cols, w, V, a, b, bits):
    """gdd_rank_wsum through the library, into NaN-filled outputs and workspace."""
    from gdd import _lib
    lib = _lib.device_lib()
    n_rows, nnz, d = rowptr.shape[0] - 1, col.shape[0], V.shape[1]
    rp, cl, wd, Vd = dev(rowptr), dev(col), dev(w), dev(V)
    ad = bd = ta = tb = None
    if a is not None:
        ad, bd = dev(a), dev(b)
        ta, tb = poisoned(n_rows, bits), poisoned(n_rows, bits)
    Y = poisoned(n_rows * d, bits).view(n_rows, d)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws, nbytes = fresh_workspace(lib, nnz, d, bits)
    p = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
    _lib.check(lib.gdd_rank_wsum(n_rows, n_cols, nnz, rp.data_ptr(), p(cl), d, p(wd), Vd.data_ptr(), p(ad), p(bd),
                                 Y.data_ptr(), p(ta), p(tb), bad.data_ptr(), ws.data_ptr(), nbytes,
                                 _lib.stream_ptr("cuda")))
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    out = {"Y": Y.cpu().numpy()}
    if a is not None:
        out.update(ta=ta.cpu().numpy(), tb=tb.cpu().numpy())
    return out


def row_sum(rows, n_rows, terms):
    out = np.zeros((n_rows,) + terms.shape[1:])
    np.add.at(out, rows, terms)
    return out


def geometry_inputs(pattern, n_cols, d):
    rowptr, col, lens = pattern_csr(R.PATTERNS[pattern], n_cols, 40 + pattern)
    rng = np.random.RandomState(1000 * pattern + 10 * d + n_cols)
    n_rows, nnz = lens.shape[0], col.shape[0]
    t = {"rowptr": rowptr, "col": col, "lens": lens, "rows": np.repeat(np.arange(n_rows), lens)}
    for name, shape in (("Q", (n_rows, d)), ("K", (n_cols, d)), ("V", (n_cols, d)), ("w", (nnz,)), ("a", (nnz,)),
                        ("b", (nnz,))):
        t[name] = rng.standard_normal(shape).astype(np.float32)
    return t


def assert_empty_rows_are_plus_zero(out, lens, skip=("s",)):
    empty = np.flatnonzero(lens == 0)
    for name, got in out.items():
        if name in skip:
            continue
        rows = got[empty]
        assert not rows.any() and not np.signbit(rows).any(), name


@pytest.mark.parametrize("d", GEOM_DIMS)
@pytest.mark.parametrize("n_cols", [50, 1])
@pytest.mark.parametrize("pattern", range(len(R.PATTERNS)))
def test_chunk_geometry_into_poisoned_buffers(pattern, n_cols, d):
    t = geometry_inputs(pattern, n_cols, d)
    rows, col, lens = t["rows"], t["col"], t["lens"]
    n_rows = lens.shape[0]
    tag = f"pattern {pattern + 1} n_cols {n_cols} d {d}"
    q, k, v = (t[x].astype(np.float64) for x in "QKV")
    q, k, v = q[rows], k[col], v[col]
    s_x, s_m = (q * k).sum(1), (np.abs(q) * np.abs(k)).sum(1)
    deg, deg1 = lens.astype(np.float64), lens[:, None].astype(np.float64)
    got = raw_rowpass(t["rowptr"], col, n_cols, t["Q"], t["K"], t["V"], QUIET_NAN)
    check(f"{tag} s", got["s"], s_x, s_m, d)
    check(f"{tag} s_sum", got["s_sum"], row_sum(rows, n_rows, s_x), row_sum(rows, n_rows, s_m), deg + d)
    check(f"{tag} SK", got["SK"], row_sum(rows, n_rows, k), row_sum(rows, n_rows, np.abs(k)), deg1 + d)
    check(f"{tag} SV", got["SV"], row_sum(rows, n_rows, v), row_sum(rows, n_rows, np.abs(v)), deg1 + d)
    check(f"{tag} A", got["A"], row_sum(rows, n_rows, s_x[:, None] * v),
          row_sum(rows, n_rows, s_m[:, None] * np.abs(v)), deg1 + d)
    assert_empty_rows_are_plus_zero(got, lens)
    w, a, b = (t[x].astype(np.float64) for x in "wab")
    for with_ab in (True, False):
        got = raw_wsum(t["rowptr"], col, n_cols, t["w"], t["V"], t["a"] if with_ab else None,
                       t["b"] if with_ab else None, QUIET_NAN)
        check(f"{tag} Y", got["Y"], row_sum(rows, n_rows, w[:, None] * v),
              row_sum(rows, n_rows, np.abs(w[:, None] * v)), deg1 + d)
        if with_ab:
            check(f"{tag} ta", got["ta"], row_sum(rows, n_rows, a), row_sum(rows, n_rows, np.abs(a)), deg + d)
            check(f"{tag} tb", got["tb"], row_sum(rows, n_rows, b), row_sum(rows, n_rows, np.abs(b)), deg + d)
        else:
            assert sorted(got) == ["Y"]
        assert_empty_rows_are_plus_zero(got, lens)


@pytest.mark.parametrize("d", GEOM_DIMS)
@pytest.mark.parametrize("pattern", range(5, len(R.PATTERNS)))
def test_cut_rows_do_not_depend_on_what_the_buffers_held(pattern, d):
    """Patterns 6 to 12 (more than one chunk each) into two differently poisoned sets of buffers."""
    t = geometry_inputs(pattern, 50, d)
    one = raw_rowpass(t["rowptr"], t["col"], 50, t["Q"], t["K"], t["V"], QUIET_NAN)
    two = raw_rowpass(t["rowptr"], t["col"], 50, t["Q"], t["K"], t["V"], OTHER_NAN)
    for name in one:
        assert np.array_equal(one[name].view(np.uint32), two[name].view(np.uint32)), name
    one = raw_wsum(t["rowptr"], t["col"], 50, t["w"], t["V"], t["a"], t["b"], QUIET_NAN)
    two = raw_wsum(t["rowptr"], t["col"], 50, t["w"], t["V"], t["a"], t["b"], OTHER_NAN)
    for name in one:
        assert np.array_equal(one[name].view(np.uint32), two[name].view(np.uint32)), name


# ---- the autograd functions against fp64 autograd of the plain definition ----------------------
AUTO_DIMS = [8, 65, 193]
ROWPASS_OUT = ("s", "s_sum", "SK", "SV", "A")
ROWPASS_CASES = {  # name -> (outputs with a cotangent, inputs that require grad)
    "all": (ROWPASS_OUT, "QKV"), "s": (("s",), "QKV"), "s_sum": (("s_sum",), "QKV"), "SK": (("SK",), "QKV"),
    "SV": (("SV",), "QKV"), "A": (("A",), "QKV"), "layer": (("s", "s_sum", "SV", "A"), "QKV"),
    "onlyQ": (ROWPASS_OUT, "Q"), "onlyK": (ROWPASS_OUT, "K"), "onlyV": (ROWPASS_OUT, "V"),
}
WSUM_OUT = ("Y", "ta", "tb")
WSUM_CASES = {  # name -> (a and b present, outputs with a cotangent)
    "all": (True, WSUM_OUT), "Y": (True, ("Y",)), "ta": (True, ("ta",)), "noab": (False, ("Y",)),
}


@pytest.fixture(scope="module")
def agraph():
    from gdd.rankformer import InteractionGraph
    u, i, n, m = R.autograd_pairs()
    g = InteractionGraph(u, i, n, m, "cuda")
    order = np.lexsort((u, i))  # the transposed orientation's entry order: by item, then user
    sides = {"users": (g.users, torch.from_numpy(u), torch.from_numpy(i)),
             "items": (g.items, torch.from_numpy(i[order]), torch.from_numpy(u[order]))}
    for side, rows, col in sides.values():
        assert torch.equal(side.rows_l.cpu(), rows) and torch.equal(side.col.cpu().long(), col)
        assert side.T.T is side and torch.equal(side.T.to_T[side.to_T].cpu(), torch.arange(side.nnz))
    dmax = max(int(np.bincount(u, minlength=n).max()), int(np.bincount(i, minlength=m).max()))
    assert dmax == n - 1
    return {"graph": g, "sides": sides, "dmax": dmax}


def fp64_grads(fn, inputs, wanted, outs_sel, cots):
    """Gradients of the plain definition ``fn(*inputs)`` (None -> zeros) for the inputs ``wanted``."""
    leaves = [t.clone().requires_grad_(k in wanted) for k, t in inputs]
    outs = fn(*leaves)
    need = [t for t in leaves if t.requires_grad]
    live = [k for k in outs_sel if outs[k].requires_grad]  # SK does not depend on Q, say
    grads = [None] * len(need)
    if live:
        grads = torch.autograd.grad([outs[k] for k in live], need, [cots[k] for k in live], allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for t, g in zip(need, grads)]


def compare_grads(tag, names, got, exact, mag, count):
    worst = 0.0
    for name, g, e, m in zip(names, got, exact, mag):
        g = torch.zeros(e.shape) if g is None else g.cpu()
        worst = max(worst, check(f"{tag} d{name}", g.numpy(), e.numpy(), m.numpy(), count))
    return worst


@pytest.mark.parametrize("d", AUTO_DIMS)
@pytest.mark.parametrize("case", list(ROWPASS_CASES))
@pytest.mark.parametrize("orient", ["users", "items"])
def test_rowpass_backward_vs_fp64_autograd(agraph, orient, case, d):
    from gdd.rankformer import _RowPass
    side, rows, col = agraph["sides"][orient]
    sel_names, wanted = ROWPASS_CASES[case]
    sel = [ROWPASS_OUT.index(k) for k in sel_names]
    g = torch.Generator().manual_seed(300 + d)
    Q, K, V = (torch.randn(r, d, generator=g) for r in (side.n_rows, side.n_cols, side.n_cols))
    shapes = ((side.nnz,), (side.n_rows,)) + ((side.n_rows, d),) * 3
    cots = [torch.randn(s, generator=g) for s in shapes]
    leaves = [t.to("cuda").requires_grad_(k in wanted) for k, t in zip("QKV", (Q, K, V))]
    outs = _RowPass.apply(*leaves, side)
    got = torch.autograd.grad([outs[k] for k in sel], [t for t in leaves if t.requires_grad],
                              [cots[k].to("cuda") for k in sel], allow_unused=True)
    agraph["graph"].check()
    if case == "SK":  # the branch dK += wsum(T, ones, gSK) alone: nothing reaches Q or V
        assert got[0] is None and got[1] is not None and got[2] is None

    def plain(Q, K, V):
        return R.plain_rowpass(rows, col, side.n_rows, Q, K, V)

    named = list(zip("QKV", (Q.double(), K.double(), V.double())))
    exact = fp64_grads(plain, named, wanted, sel, [c.double() for c in cots])
    mag = fp64_grads(plain, [(k, t.abs()) for k, t in named], wanted, sel, [c.double().abs() for c in cots])
    compare_grads(f"rowpass {orient} {case} d={d}:", wanted, got, exact, mag, agraph["dmax"] + d + 4)


@pytest.mark.parametrize("d", AUTO_DIMS)
@pytest.mark.parametrize("case", list(WSUM_CASES))
@pytest.mark.parametrize("orient", ["users", "items"])
def test_wsum_backward_vs_fp64_autograd(agraph, orient, case, d):
    from gdd.rankformer import _WSum
    side, rows, col = agraph["sides"][orient]
    with_ab, sel_names = WSUM_CASES[case]
    sel = [WSUM_OUT.index(k) for k in sel_names]
    wanted = "wVab" if with_ab else "wV"
    g = torch.Generator().manual_seed(400 + d)
    w, a, b = (torch.randn(side.nnz, generator=g) for _ in range(3))
    V = torch.randn(side.n_cols, d, generator=g)
    cots = [torch.randn(side.n_rows, d, generator=g), torch.randn(side.n_rows, generator=g),
            torch.randn(side.n_rows, generator=g)]
    host = [w, V] + ([a, b] if with_ab else [])
    leaves = [t.to("cuda").requires_grad_(True) for t in host]
    outs = _WSum.apply(*(leaves + [None] * (4 - len(leaves))), side)
    if not with_ab:
        assert outs[1].numel() == 0 and outs[2].numel() == 0
    got = torch.autograd.grad([outs[k] for k in sel], leaves, [cots[k].to("cuda") for k in sel], allow_unused=True)
    agraph["graph"].check()

    def plain(w, V, a=None, b=None):
        return R.plain_wsum(rows, col, side.n_rows, w, V, a, b)

    named = list(zip(wanted, (t.double() for t in host)))
    exact = fp64_grads(plain, named, wanted, sel, [c.double() for c in cots])
    mag = fp64_grads(plain, [(k, t.abs()) for k, t in named], wanted, sel, [c.double().abs() for c in cots])
    compare_grads(f"wsum {orient} {case} d={d}:", wanted, got, exact, mag, agraph["dmax"] + d + 4)


# ---- the layer against the second fixture -------------------------------------------------------
@pytest.fixture(scope="module", params=list(R.MORE_CASES))
def more(request):
    from gdd.rankformer import InteractionGraph
    c = R.load_more_case(request.param)
    c["graph"] = InteractionGraph(c["u"], c["i"], int(c["n"]), int(c["m"]), "cuda")
    return c


def more_run(c):
    """(z, dL/dx) on the device for L = sum(z * W): the layer, or for ``layers`` > 1 the teacher's
    computer() with its embedding weights set to x."""
    from gdd.rankformer import RankformerLayer, RankformerTeacher
    g, n = c["graph"], int(c["n"])
    x, W = dev(c["x"].astype(np.float32)), dev(c["W"].astype(np.float32))
    if c["layers"] == 1:
        x.requires_grad_(True)
        z = RankformerLayer(c["alpha"], c["clamp"])(x, g)
        (z * W).sum().backward()
        grad = x.grad
    else:
        model = RankformerTeacher(g, hidden_dim=x.shape[1], rankformer_layers=c["layers"], rankformer_tau=R.TAU,
                                  rankformer_alpha=c["alpha"], rankformer_clamp_value=c["clamp"])
        with torch.no_grad():
            model.embedding_user.weight.copy_(x[:n])
            model.embedding_item.weight.copy_(x[n:])
        z = torch.cat(model.computer(), 0)
        (z * W).sum().backward()
        grad = torch.cat([model.embedding_user.weight.grad, model.embedding_item.weight.grad], 0)
    g.check()
    return z.detach(), grad.detach()


def test_layer_vs_reference_on_the_second_fixture(more):
    z1, g1 = more_run(more)
    z2, g2 = more_run(more)
    failed = []
    for what, got, key in (("forward", z1, "z"), ("gradient", g1, "g")):
        ref_err = float(more[key + "32_err"])
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - more[key + "64"]).max())
        print(f"{more['name']} {what}: err {err:.3e}, reference fp32 err {ref_err:.3e}, ratio {err / ref_err:.2f}")
        if not err <= 4 * ref_err:
            failed.append((what, err, ref_err))
    assert not failed, failed
    assert torch.equal(z1, z2) and torch.equal(g1, g2)


# ---- small things -------------------------------------------------------------------------------
def test_graph_without_pairs():
    from gdd.rankformer import InteractionGraph, RankformerLayer
    n, m, d = 9, 7, 8
    g = InteractionGraph([], [], n, m, "cuda")
    assert g.E == 0 and g.users.nnz == 0 and g.items.nnz == 0
    rng = np.random.RandomState(17)
    x32 = (0.1 * rng.standard_normal((n + m, d))).astype(np.float32)
    W32 = rng.standard_normal((n + m, d)).astype(np.float32)
    x = dev(x32).requires_grad_(True)
    z = RankformerLayer(2.0, 0.0)(x, g)
    (z * dev(W32)).sum().backward()
    g.check()
    M = torch.zeros(n, m, dtype=torch.float64)
    x64, W64 = torch.from_numpy(x32.astype(np.float64)), torch.from_numpy(W32.astype(np.float64))
    count = max(n, m) + d + 4
    check("no pairs forward", z.detach().cpu().numpy(), R.dense_rankformer(x64, M).numpy(),
          R.dense_rankformer_terms(x64, M).numpy(), count)
    J = torch.autograd.functional.jacobian(lambda t: R.dense_rankformer(t, M), x64)  # [n+m, d, n+m, d]
    exact = torch.einsum("rf,rfke->ke", W64, J)
    mag = torch.einsum("rf,rfke->ke", W64.abs(), J.abs())
    check("no pairs gradient", x.grad.cpu().numpy(), exact.numpy(), mag.numpy(), count)


def test_sampler_returns_beside_a_user_that_holds_every_item():
    from gdd.rankformer import InteractionGraph, NegativeSampler
    c = R.load_case("small")
    n, m = int(c["n"]), int(c["m"])
    assert np.bincount(c["u"], minlength=n)[1] == m  # user 1 has no negative item
    g = InteractionGraph(c["u"], c["i"], n, m, "cuda")
    pick = torch.randint(0, g.E, (2048,), generator=torch.Generator().manual_seed(2))
    u = g.train_u[pick.to("cuda")]
    assert int((u == 1).sum()) > 0
    j = NegativeSampler(g, seed=3)(u)
    assert j.shape == u.shape and int(j.min()) >= 0 and int(j.max()) < m
    pairs = set(zip(c["u"].tolist(), c["i"].tolist()))
    assert not any((a, b) in pairs for a, b in zip(u.tolist(), j.tolist()) if a != 1)
