"""The training-path COO kernels (k_batched_coo_spmv / _edge / _spmm / _sddmm, dpcg_setup.hip) and COO -> CSR (dpcg_coo.hip) at their
edges, against the numpy restatement (tests/coo_restatement.py) on the cases of tests/coo_edge_cases.py.

1.  The raw entry points, through `_lib`: all four kernels, both `transpose` values, every case -- the four capped grids with their stride
    loops entered, panel widths around the 64 lanes of a wave, five samples with empty ones among them, 300 triples on one entry, triples
    out of range, explicit zeros over inf and NaN, nnz = 0.  spmv, spmm and sddmm are held, element by element, to the a-priori bound
    gamma_m S of the restatement (any summation order, fused or not; nothing measured): it lies below a quarter of the smallest term of
    every output and the restatement with one defect built in lies >= 10 bounds away (tests/test_coo_edges_host.py), so a wrong batch
    offset, a lost last strided element, a dropped duplicate or a lost panel column fails here.  edge is one fp32 product: bit for bit.
2.  The autograd functions behind `sparse_matvec_mul` / `sparse_matmat_mul`: gradients against the restatement with the same bounds,
    one `requires_grad` at a time, a strided upstream gradient, fp64 in and out, indices that do not fit int32; `frobenius_loss` and
    `inverse_loss` on two matrices of different size against an fp64 dense restatement with the project's tolerances for that
    comparison (test_inverse_loss_on_sparse_operands: rtol 2e-6 on the loss, rtol 2e-4 / atol 1e-6 on the gradient).
3.  COO -> CSR bit for bit -- pattern, values, count -- also where only the storage order of duplicates decides the sum, at n = 1,
    2^k and 2^k + 1, on one run of 5000, back to back at different sizes, on a side stream, and after a refused call.
"""

import ctypes as C_

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import coo_edge_cases as C
import coo_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else C_.c_void_p(t.data_ptr())


def stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def host(t):
    return t.detach().cpu().numpy()


def held(true, got, label):
    """every element within the restatement's a-priori bound; prints the distance in bounds before it asserts"""
    far = C.distance(true, host(got) if isinstance(got, torch.Tensor) else got)
    print(f"{label}: {far:.3g} bounds from the restatement (m <= {int(true.m.max(initial=0))})")
    assert far <= 1.0, (label, far)


def edge_fp32(c, a, other, transpose):
    """np.float32(a) * np.float32(c) per triple, 0 for a triple out of range"""
    b, r, s, ok = R._triples(c.idx, c.batch, c.dof, transpose)
    want = np.zeros(c.nnz, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        want[ok] = a[b[ok], r[ok]] * other[b[ok], s[ok]]
    assert want.dtype == np.float32
    return want


def same_bits(got, want):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    nan = np.isnan(want)
    word = np.uint32 if want.dtype == np.float32 else np.uint64
    return got.dtype == want.dtype and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(word), want[~nan].view(word))


# ---- 1. raw entry points ------------------------------------------------------------------------------------------------------------
def raw(D, op, c, transpose, first, second=None, ncols=0):
    """one call of dpcg_batched_coo_<op> on a case; the output starts as NaN, so an element the call leaves alone shows"""
    lib = D._lib.lib()
    idx, feat = dev(c.idx), dev(c.feat)
    t = 1 if transpose else 0
    if op == "spmv":
        out = torch.full((c.batch, c.dof), float("nan"), device="cuda")
        st = lib.dpcg_batched_coo_spmv(c.nnz, ptr(idx), ptr(feat), c.batch, c.dof, ptr(first), ptr(out), t, stream())
    elif op == "edge":
        out = torch.full((c.nnz,), float("nan"), device="cuda")
        st = lib.dpcg_batched_coo_edge(c.nnz, ptr(idx), c.batch, c.dof, ptr(first), ptr(second), ptr(out), t, stream())
    elif op == "spmm":
        out = torch.full((c.batch, c.dof, ncols), float("nan"), device="cuda")
        st = lib.dpcg_batched_coo_spmm(c.nnz, ptr(idx), ptr(feat), c.batch, c.dof, ncols, ptr(first), ptr(out), t, stream())
    else:
        out = torch.full((c.nnz,), float("nan"), device="cuda")
        st = lib.dpcg_batched_coo_sddmm(c.nnz, ptr(idx), c.batch, c.dof, ncols, ptr(first), ptr(second), ptr(out), t, stream())
    assert st == D._lib.OK, (op, c.name, st, lib.dpcg_last_error())
    torch.cuda.synchronize()
    return host(out)


@pytest.mark.parametrize("name", list(C.CASES))
def test_spmv_and_edge_raw(D, name):
    c = C.case(name)
    vec, g = C.vectors(name)
    ok, _ = C.valid_part(c)
    for transpose in C.TRANSPOSES:
        y = raw(D, "spmv", c, transpose, dev(vec))
        held(C.restated(name, "spmv", transpose), y, f"{name} spmv transpose={int(transpose)}")
        e = raw(D, "edge", c, transpose, dev(g), dev(vec))
        want = edge_fp32(c, g, vec, transpose)
        assert same_bits(want, C.restated(name, "edge", transpose).value.astype(np.float32))       # the exact product, rounded once
        assert same_bits(e, want), (name, transpose, int(np.sum(e != want)))
        assert np.all(e[~ok].view(np.uint32) == 0)                                                  # out of range: exactly +0.0
        if c.nnz == 0:
            assert np.all(y.view(np.uint32) == 0)
    if name == "out_of_range":
        assert (~ok).sum() == 8
    if name == "explicit_zeros":
        assert np.isnan(y).any() and np.isfinite(y).any()        # spmv has no zero test: 0 * inf = NaN, as IEEE has it


@pytest.mark.parametrize("name", list(C.CASES))
def test_spmm_and_sddmm_raw(D, name):
    c = C.case(name)
    ok, _ = C.valid_part(c)
    for ncols in c.widths:
        panel, g = C.panels(name, ncols)
        for transpose in C.TRANSPOSES:
            Y = raw(D, "spmm", c, transpose, dev(panel), ncols=ncols)
            held(C.restated(name, "spmm", transpose, ncols), Y, f"{name} spmm[{ncols}] transpose={int(transpose)}")
            d = raw(D, "sddmm", c, transpose, dev(g), dev(panel), ncols=ncols)
            held(C.restated(name, "sddmm", transpose, ncols), d, f"{name} sddmm[{ncols}] transpose={int(transpose)}")
            assert np.all(d[~ok].view(np.uint32) == 0)
            if c.nnz == 0:
                assert np.all(Y.view(np.uint32) == 0)
            if name == "explicit_zeros":
                assert np.isfinite(Y).all() and not np.isfinite(d).all()        # the zero test is spmm's alone


def test_bad_arguments_are_refused(D):
    lib, INV = D._lib.lib(), D._lib.ERR_INVALID
    c = C.case("batch_offsets")
    idx, feat = dev(c.idx), dev(c.feat)
    vec, out, e = dev(C.vectors(c.name)[0]), torch.zeros(c.batch, c.dof, device="cuda"), torch.zeros(c.nnz, device="cuda")
    panel, pout = dev(C.panels(c.name, 5)[0]), torch.zeros(c.batch, c.dof, 5, device="cuda")
    s = stream()

    def spmv(nnz=c.nnz, idx=idx, feat=feat, batch=c.batch, dof=c.dof, vec=vec, out=out):
        return lib.dpcg_batched_coo_spmv(nnz, ptr(idx), ptr(feat), batch, dof, ptr(vec), ptr(out), 0, s)

    def edge(nnz=c.nnz, idx=idx, batch=c.batch, dof=c.dof, a=vec, b=vec, out=e):
        return lib.dpcg_batched_coo_edge(nnz, ptr(idx), batch, dof, ptr(a), ptr(b), ptr(out), 0, s)

    def spmm(nnz=c.nnz, idx=idx, feat=feat, batch=c.batch, dof=c.dof, ncols=5, panel=panel, out=pout):
        return lib.dpcg_batched_coo_spmm(nnz, ptr(idx), ptr(feat), batch, dof, ncols, ptr(panel), ptr(out), 0, s)

    def sddmm(nnz=c.nnz, idx=idx, batch=c.batch, dof=c.dof, ncols=5, g=panel, panel=panel, out=e):
        return lib.dpcg_batched_coo_sddmm(nnz, ptr(idx), batch, dof, ncols, ptr(g), ptr(panel), ptr(out), 0, s)

    for fn in (spmv, edge, spmm, sddmm):
        assert fn() == D._lib.OK
        assert fn(batch=0) == INV and fn(dof=0) == INV and fn(nnz=-1) == INV and fn(idx=None) == INV and fn(out=None) == INV
        assert b"bad arguments" in lib.dpcg_last_error()
    assert spmm(ncols=0) == INV and sddmm(ncols=0) == INV
    assert spmv(feat=None) == INV and spmv(vec=None) == INV and spmm(feat=None) == INV and spmm(panel=None) == INV
    assert edge(a=None) == INV and edge(b=None) == INV and sddmm(g=None) == INV and sddmm(panel=None) == INV
    # nnz = 0 needs neither triples nor, for edge and sddmm, an output
    assert spmv(nnz=0, idx=None, feat=None) == D._lib.OK and spmm(nnz=0, idx=None, feat=None) == D._lib.OK
    assert edge(nnz=0, idx=None, a=None, b=None, out=None) == D._lib.OK and sddmm(nnz=0, idx=None, g=None, panel=None, out=None) == D._lib.OK
    torch.cuda.synchronize()
    assert not out.any() and not pout.any()              # spmv and spmm with nnz = 0 still clear their output


# ---- 2. the autograd functions ------------------------------------------------------------------------------------------------------
def sparse_batch(c, feat):
    from deeppreconditioning_amd.utils import SparseBatch
    return SparseBatch(feat, dev(c.idx), [c.dof, c.dof], c.batch)


@pytest.mark.parametrize("name", C.GRAD_CASES)
def test_matvec_gradients(D, name):
    from deeppreconditioning_amd.utils import sparse_matvec_mul
    c = C.case(name)
    vec_h, g_h = C.vectors(name)
    g = dev(g_h)
    g_strided = dev(np.ascontiguousarray(g_h.T)).t()
    assert not g_strided.is_contiguous() and torch.equal(g_strided, g)
    for transpose in C.TRANSPOSES:
        label = f"{name} matvec transpose={int(transpose)}"
        want_y, want_gv = C.restated(name, "spmv", transpose), C.restated(name, "spmv", not transpose, 0, True)
        want_gf = edge_fp32(c, g_h, vec_h, transpose)
        feat, vec = dev(c.feat).reshape(-1, 1).requires_grad_(True), dev(vec_h).requires_grad_(True)
        y = sparse_matvec_mul(sparse_batch(c, feat), vec, transpose)
        assert y.dtype == torch.float32
        held(want_y, y, label)
        gf, gv = torch.autograd.grad(y, (feat, vec), grad_outputs=g)
        assert gf.shape == feat.shape and same_bits(host(gf), want_gf)
        held(want_gv, gv, label + " d/dvec")
        # one requires_grad at a time: the other gradient is None, the computed one unchanged
        feat1, vec1 = dev(c.feat).reshape(-1, 1).requires_grad_(True), dev(vec_h)
        sparse_matvec_mul(sparse_batch(c, feat1), vec1, transpose).backward(g)
        assert vec1.grad is None and same_bits(host(feat1.grad), want_gf)
        feat2, vec2 = dev(c.feat).reshape(-1, 1), dev(vec_h).requires_grad_(True)
        sparse_matvec_mul(sparse_batch(c, feat2), vec2, transpose).backward(g)
        assert feat2.grad is None
        held(want_gv, vec2.grad, label + " d/dvec alone")
        # a strided upstream gradient
        gf, gv = torch.autograd.grad(sparse_matvec_mul(sparse_batch(c, feat), vec, transpose), (feat, vec), grad_outputs=g_strided)
        assert same_bits(host(gf), want_gf)
        held(want_gv, gv, label + " d/dvec, strided upstream gradient")
        # fp64 in: fp64 out and an fp64 gradient (the values are fp32-exact, so the bounds hold unchanged)
        vec64 = dev(vec_h.astype(np.float64)).requires_grad_(True)
        y64 = sparse_matvec_mul(sparse_batch(c, feat), vec64, transpose)
        (gv64,) = torch.autograd.grad(y64, (vec64,), grad_outputs=g.double())
        assert y64.dtype == torch.float64 and gv64.dtype == torch.float64
        held(want_y, y64, label + " fp64")
        held(want_gv, gv64, label + " fp64 d/dvec")


@pytest.mark.parametrize("name", C.GRAD_CASES)
def test_matmat_gradients(D, name):
    from deeppreconditioning_amd.utils import sparse_matmat_mul
    c = C.case(name)
    for ncols in c.widths:
        panel_h, g_h = C.panels(name, ncols)
        g = dev(g_h)
        g_strided = dev(np.repeat(g_h, 2, axis=2))[:, :, ::2]                  # every other column of a panel twice as wide
        assert not g_strided.is_contiguous() and torch.equal(g_strided, g)
        for transpose in C.TRANSPOSES:
            label = f"{name} matmat[{ncols}] transpose={int(transpose)}"
            want_y, want_gp = C.restated(name, "spmm", transpose, ncols), C.restated(name, "spmm", not transpose, ncols, True)
            want_gf = C.restated(name, "sddmm", transpose, ncols)
            feat, panel = dev(c.feat).reshape(-1, 1).requires_grad_(True), dev(panel_h).requires_grad_(True)
            y = sparse_matmat_mul(sparse_batch(c, feat), panel, transpose)
            assert y.dtype == torch.float32
            held(want_y, y, label)
            gf, gp = torch.autograd.grad(y, (feat, panel), grad_outputs=g)
            held(want_gf, gf.reshape(-1), label + " d/dfeat")
            held(want_gp, gp, label + " d/dpanel")
            feat1, panel1 = dev(c.feat).reshape(-1, 1).requires_grad_(True), dev(panel_h)
            sparse_matmat_mul(sparse_batch(c, feat1), panel1, transpose).backward(g)
            assert panel1.grad is None and same_bits(host(feat1.grad), host(gf))        # the wave sum has a fixed order
            feat2, panel2 = dev(c.feat).reshape(-1, 1), dev(panel_h).requires_grad_(True)
            sparse_matmat_mul(sparse_batch(c, feat2), panel2, transpose).backward(g)
            assert feat2.grad is None
            held(want_gp, panel2.grad, label + " d/dpanel alone")
            gf_s, gp_s = torch.autograd.grad(sparse_matmat_mul(sparse_batch(c, feat), panel, transpose), (feat, panel),
                                             grad_outputs=g_strided)
            assert same_bits(host(gf_s), host(gf))
            held(want_gp, gp_s, label + " d/dpanel, strided upstream gradient")
            # the panel's dtype comes back, as sparse_matvec_mul returns its vectors'
            panel64 = dev(panel_h.astype(np.float64)).requires_grad_(True)
            y64 = sparse_matmat_mul(sparse_batch(c, feat), panel64, transpose)
            (gp64,) = torch.autograd.grad(y64, (panel64,), grad_outputs=g.double())
            assert y64.dtype == torch.float64 and gp64.dtype == torch.float64
            held(want_y, y64, label + " fp64")
            held(want_gp, gp64, label + " fp64 d/dpanel")


@pytest.mark.parametrize("bad", [3 + 2 ** 32, -2 ** 31 - 1])
def test_an_index_that_does_not_fit_int32_is_refused(D, bad):
    """`.to(torch.int32)` wraps 3 + 2**32 to the valid index 3"""
    from deeppreconditioning_amd import io as dio
    from deeppreconditioning_amd.utils import sparse_matmat_mul, sparse_matvec_mul
    c = C.case("batch_offsets")
    vec, panel = dev(C.vectors(c.name)[0]), dev(C.panels(c.name, 5)[0])
    wide = dev(c.idx.astype(np.int64))
    batch = sparse_batch(c, dev(c.feat).reshape(-1, 1))
    batch.indices = wide                                  # int64 indices that fit are narrowed as before
    held(C.restated(c.name, "spmv", False), sparse_matvec_mul(batch, vec, False), "int64 indices, spmv")
    held(C.restated(c.name, "spmm", True, 5), sparse_matmat_mul(batch, panel, True), "int64 indices, spmm")
    for column in range(3):
        spoiled = wide.clone()
        spoiled[7, column] = bad
        batch.indices = spoiled
        with pytest.raises(ValueError, match="does not fit int32"):
            sparse_matvec_mul(batch, vec, False)
        with pytest.raises(ValueError, match="does not fit int32"):
            sparse_matmat_mul(batch, panel, False)
    rows, cols, vals, n = C.coo_case("n256")
    for as_tensor in (False, True):
        for spoil_rows in (True, False):
            r, s = rows.copy(), cols.copy()
            (r if spoil_rows else s)[5] = bad
            with pytest.raises(ValueError, match="does not fit int32"):
                dio.coo_to_csr_device(dev(r) if as_tensor else r, dev(s) if as_tensor else s, vals, n)
    assert_csr(dio.coo_to_csr_device(rows, cols, vals, n), "n256")


# -- the losses, on two matrices of different size
def loss_inputs():
    rng = np.random.default_rng(301)
    mats = []
    for n in (23, 16):
        M = sp.random(n, n, density=0.2, random_state=rng, data_rvs=lambda k: rng.uniform(-1.0, 1.0, k))
        M = (M + M.T).tocsr()
        M = M + sp.diags(np.abs(M).sum(axis=1).A1 + 1.0)
        mats.append(M.tocsr().astype(np.float32).astype(np.float64))
    return mats, 26


def dense_losses(idx, a_feat, l_feat, batch, dof, x, rhs):
    """fp64, dense, on the CPU: mean_b || L L^T A - I ||_F and sum_b || L L^T x - rhs ||_2 with autograd through both"""
    b, r, c = (torch.from_numpy(idx[:, i].astype(np.int64)) for i in range(3))
    L = torch.zeros(batch, dof, dof, dtype=torch.float64).index_put((b, r, c), l_feat, accumulate=True)
    A = torch.zeros(batch, dof, dof, dtype=torch.float64).index_put((b, r, c), a_feat, accumulate=True)
    A = A + torch.tril(A, -1).transpose(1, 2)
    inverse = torch.linalg.matrix_norm(L @ L.transpose(1, 2) @ A - torch.eye(dof, dtype=torch.float64)).mean()
    y = (L @ (L.transpose(1, 2) @ x.unsqueeze(-1))).squeeze(-1)
    frobenius = torch.linalg.vector_norm(y - rhs, ord=2, dim=1).sum()
    return inverse, frobenius


def test_losses_on_two_matrices_of_different_size(D):
    from deeppreconditioning_amd import metrics
    from deeppreconditioning_amd import model as mdl
    mats, dof = loss_inputs()
    systems, sizes = mdl.tril_batch_from_csr(mats, dof_max=dof, device="cuda")
    assert sizes == (23, 16) and systems.spatial_shape == [dof, dof] and systems.batch_size == 2
    idx = host(systems.indices)
    assert np.sum(idx[:, 0] == 1) > 0 and idx[idx[:, 0] == 1][:, 1].max() == dof - 1          # padded with identity rows
    rng = np.random.default_rng(302)
    l_h = (host(systems.features) * 0.2 + rng.uniform(0.05, 0.15, systems.features.shape)).astype(np.float32)
    x_h, rhs_h = C.values(rng, (2, dof)), C.values(rng, (2, dof))
    l64 = torch.from_numpy(l_h.astype(np.float64).reshape(-1)).requires_grad_(True)
    inv64, fro64 = dense_losses(idx, torch.from_numpy(host(systems.features).astype(np.float64).reshape(-1)), l64, 2, dof,
                                torch.from_numpy(x_h.astype(np.float64)), torch.from_numpy(rhs_h.astype(np.float64)))
    (inv_grad,) = torch.autograd.grad(inv64, l64, retain_graph=True)
    (fro_grad,) = torch.autograd.grad(fro64, l64)

    def compare(what, loss, grad, want, want_grad):
        got, got_grad = float(loss.detach()), host(grad).reshape(-1).astype(np.float64)
        err = np.abs(got_grad - want_grad.numpy())
        print(f"{what}: loss {got!r} against {float(want)!r} (relative {abs(got - float(want)) / float(want):.3g}); gradient off by up "
              f"to {err.max():.3g} absolutely, {np.max(err / np.maximum(np.abs(want_grad.numpy()), 1e-300)):.3g} relatively")
        np.testing.assert_allclose(got, float(want), rtol=2e-6)
        np.testing.assert_allclose(got_grad, want_grad.numpy(), rtol=2e-4, atol=1e-6)

    for width in (1, 7, dof, dof + 5):
        assert width in (1, dof, dof + 5) or dof % width != 0
        feats = dev(l_h).requires_grad_(True)
        loss = metrics.inverse_loss(systems, systems.replace_feature(feats), panel_columns=width)
        (grad,) = torch.autograd.grad(loss, feats)
        compare(f"inverse_loss, panels of {width}", loss, grad, inv64.detach(), inv_grad)
        with torch.no_grad():
            np.testing.assert_allclose(float(metrics.inverse_loss(systems, systems.replace_feature(dev(l_h)), panel_columns=width)),
                                       float(inv64), rtol=2e-6)
    feats = dev(l_h).requires_grad_(True)
    loss = metrics.frobenius_loss(systems.replace_feature(feats), dev(x_h), dev(rhs_h))
    (grad,) = torch.autograd.grad(loss, feats)
    compare("frobenius_loss", loss, grad, fro64.detach(), fro_grad)


# ---- 3. COO -> CSR ---------------------------------------------------------------------------------------------------------------------
def assert_csr(got, name):
    rowptr, col, val = (host(t) for t in got)
    want = C.coo_restated(name)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float64
    assert len(col) == len(want[1]) == len(val), (name, len(col), len(want[1]))          # nnz_out
    assert np.array_equal(rowptr, want[0]) and np.array_equal(col, want[1]), name
    differ = val.view(np.uint64) != want[2].view(np.uint64)
    assert not differ.any(), (name, int(differ.sum()), val[differ][:4], want[2][differ][:4])


@pytest.mark.parametrize("name", list(C.COO_CASES))
def test_coo_to_csr_bit_for_bit(D, name):
    from deeppreconditioning_amd import io as dio
    rows, cols, vals, n = C.coo_case(name)
    assert_csr(dio.coo_to_csr_device(rows, cols, vals, n), name)
    # the raw entry point: the count comes back through nnz_out
    r, s, v = dev(rows.astype(np.int32)), dev(cols.astype(np.int32)), dev(vals)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    col, val = torch.empty(len(rows), dtype=torch.int32, device="cuda"), torch.empty(len(rows), dtype=torch.float64, device="cuda")
    count = C_.c_int64(-1)
    assert D._lib.lib().dpcg_coo_to_csr(n, len(rows), ptr(r), ptr(s), ptr(v), ptr(rowptr), ptr(col), ptr(val), C_.byref(count),
                                        stream()) == D._lib.OK
    assert count.value == len(C.coo_restated(name)[1])
    assert_csr((rowptr, col[:count.value], val[:count.value]), name)


def test_coo_to_csr_back_to_back_at_different_sizes(D):
    """the scratch blocks of one call are cached and handed to the next"""
    from deeppreconditioning_amd import io as dio
    for name in ("integers", "nnz1", "storage_order", "n1", "one_run", "integers", "n257", "storage_order"):
        assert_csr(dio.coo_to_csr_device(*C.coo_case(name)), name)


def test_coo_to_csr_on_a_side_stream(D):
    """the call directly follows, on the same side stream, the kernels that produce its inputs (behind a product that keeps the stream
    busy): it has to order itself on that stream, not on the default one"""
    from deeppreconditioning_amd import io as dio
    name = "storage_order"
    rows, cols, vals, n = C.coo_case(name)
    r0, s0, half = dev(rows.astype(np.int32)), dev(cols.astype(np.int32)), dev(vals * 0.5)
    busy = torch.full((2048, 2048), 2.0 ** -12, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        late = (busy @ busy @ busy)[0, 0].to(torch.int32)        # 2048^2 * 2^-36 = 2^-14 -> 0, but only once the products are done
        r, s, v = r0 + late, s0 + late, half * 2.0 + late
        got = dio.coo_to_csr_device(r, s, v, n)
        side.synchronize()
    assert_csr(got, name)
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream


def test_coo_to_csr_refuses_an_index_out_of_range_and_recovers(D):
    from deeppreconditioning_amd import io as dio
    rows, cols, vals, n = C.coo_case("n256")
    for spoil_rows, bad in ((True, -1), (False, -1), (False, n), (True, n), (False, C.INT32_MAX), (True, C.INT32_MIN)):
        r, s = rows.copy(), cols.copy()
        (r if spoil_rows else s)[len(r) // 2] = bad
        with pytest.raises(D._lib.DpcgError, match="index out of range") as info:
            dio.coo_to_csr_device(r, s, vals, n)
        assert info.value.status == D._lib.ERR_INVALID
        assert_csr(dio.coo_to_csr_device(rows, cols, vals, n), "n256")           # the call after it is correct
