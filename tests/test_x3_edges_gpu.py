"""The three-part fp32 GEMM (csrc/mrec_gemm_x3.hip: the VAR & 4 instantiations of the body in csrc/mrec_gemm.h, EPI_F32 and EPI_X3,
k_x3_pair + k_x3_fold_cols, k_x3_post) at both tile shapes, every edge and split.  Cases and generators: _x3_edge_cases.py (checked
without a device by test_x3_edges.py).

  exact families   integer inputs whose every part product and partial sum stays below 2^24: the result IS the integer product,
                   bit for bit -- a K-tile dropped, doubled or read from the wrong part or offset in any of the six segments shows
  general inputs   the inputs and bounds of tests/test_x3_gemm_gpu.py, nothing wider: forms 0 and 1 |gpu - f64| <= 6 . 2^-24 sum |a| |b|
                   per element; form 2 the worst ratio e <= max(8 u, 2 e32 + 2 u) with e32 that of ops.dense32_bwd_weight on the
                   same data; column sums within 64 . 2^-24 sum |dx| of the float64 sums of the GPU's own output
  fused ends       x3_fwd / x3_dgrad: bit-equal to the host's fp32 bias + ReLU (ReLU mask . scale) of the plain product, which the
                   checks above hold; parts images bit-equal to the host's split of the fp32 output, their padding still zero

Every output is the [:rows, :W] window of a NaN-filled buffer two rows taller and 6 or 8 columns wider (all four classes of
(W % 4, ld % 4)): afterwards the window holds no NaN and everything outside it still does.  Every case written for one tile
shape asks ops.x3_tile_rows, every split case mrec_x3_gemm_dgrad_workspace_bytes, and FAILS when the rule has moved."""
import numpy as np
import pytest
import torch

import _x3_edge_cases as T

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = T.U
INPUTS = ["general"] + T.FAMILIES


# ---- operands, guarded outputs ---------------------------------------------------------------------------------------------------------
def _inputs(kind, form, p, red, q):
    return T.general_inputs(form, p, red, q) if kind == "general" else T.exact_inputs(kind, form, p, red, q)


def _images(form, A, B, dev):
    Pm, Qm = T.operands(form, A, B)
    return T.parts_image(Pm).to(dev), T.parts_image(Qm).to(dev)


def _window(rows, W, pad, dev):
    buf = torch.full((rows + 2, W + pad), NAN, dtype=torch.float32, device=dev)
    return buf, buf[:rows, :W]


def _slab_window(S, rows, W, pad, dev):
    """[S, rows, W] whose slabs are rows . ld apart (what form 2 writes), as a window of a [S . rows + 2, W + pad] buffer"""
    buf = torch.full((S * rows + 2, W + pad), NAN, dtype=torch.float32, device=dev)
    return buf, buf[:S * rows].view(S, rows, W + pad)[:, :, :W]


def _read(buf, rows, W, what):
    g = buf.cpu().numpy()
    out = g[:rows, :W]
    assert np.isnan(g[rows:, :]).all(), f"{what}: rows below the window written"
    assert np.isnan(g[:rows, W:]).all(), (f"{what}: columns right of the window written "
                                          f"(W % 4, ld % 4) = ({W % 4}, {g.shape[1] % 4}): {sorted(set(np.nonzero(~np.isnan(g[:rows, W:]))[1] + W))}")
    assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} elements of the window never written"
    return np.ascontiguousarray(out)


def _guarded(shape, dev):
    """contiguous fp32 NaN tensor of `shape` with NaN guards before and behind"""
    n, guard = int(np.prod(shape)), 2 * shape[-1] + 8
    guard += -guard % 4
    buf = torch.full((n + 2 * guard,), NAN, dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n].view(shape)


def _read_guarded(buf, win, what):
    g = buf.cpu().numpy()
    guard = (g.size - win.numel()) // 2
    assert np.isnan(g[:guard]).all() and np.isnan(g[guard + win.numel():]).all(), f"{what}: written outside its extent"
    out = g[guard:guard + win.numel()].reshape(tuple(win.shape))
    assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} elements never written"
    return out


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _check_parts(img, out, what):
    """the image == the host's three-part split of the fp32 output `out`, bit for bit, and zero in all of its padding"""
    assert torch.equal(_bits(img), _bits(T.parts_image(out))), f"{what}: parts image differs from the host's split of the output (or its padding is not zero)"


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------
def _ratio(got, A, B):
    a64, b64 = A.astype(np.float64), B.astype(np.float64)
    return float((np.abs(got.astype(np.float64) - a64 @ b64) / (np.abs(a64) @ np.abs(b64))).max())


def _check(kind, got, A, B, what):
    """forms 0 and 1 (and exact inputs in any form)"""
    if kind != "general":
        ref = A.astype(np.float64) @ B.astype(np.float64)              # integers below 2^24: exact in float64 as in int64
        bad = got.astype(np.float64) != ref
        assert not bad.any(), (f"{what} exact family {kind}: {int(bad.sum())} of {bad.size} elements differ from the integer product, "
                               f"first at {tuple(np.argwhere(bad)[0])}: {got[bad][0]} for {ref[bad][0]}")
    else:
        r = _ratio(got, A, B)
        assert r <= 6 * U, f"{what}: worst error {r / U:.3g} u of sum |a| |b| (bound 6 u)"


def _e32(A, B, dev):
    """the exact-fp32 kernel's worst ratio on the weight gradient of the same data (x = A^T, dy = B)"""
    from mindrec_amd import ops
    x, dy = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev), torch.from_numpy(B).to(dev)
    M, K, N = x.shape[0], x.shape[1], dy.shape[1]
    S32 = ops.dense32_bwd_weight_slabs(M, K, N)
    w32 = ops.dense32_bwd_weight(x, dy, torch.empty((S32, K, N), dtype=torch.float32, device=dev)).cpu().numpy().astype(np.float64).sum(0)
    return _ratio(w32, A, B)


def _check_slab_sum(kind, slabs, A, B, e32, what):
    tot = slabs.astype(np.float64).sum(0)
    if kind != "general":
        return _check(kind, tot, A, B, what)
    e = _ratio(tot, A, B)
    assert e <= max(8 * U, 2 * e32 + 2 * U), f"{what}: worst error {e / U:.3g} u, the exact-fp32 kernel's {e32 / U:.3g} u"


def _check_colsum(cs, dx, what):
    G = cs.shape[0]
    ref = np.stack([dx[g * 64:(g + 1) * 64].astype(np.float64).sum(0) for g in range(G)])
    mag = np.stack([np.abs(dx[g * 64:(g + 1) * 64]).astype(np.float64).sum(0) for g in range(G)])
    bad = np.abs(cs.astype(np.float64) - ref) > 64 * U * mag
    assert not bad.any(), f"{what}: column sums of {int(bad.sum())} (group, column) pairs outside 64 u sum |dx|, first {tuple(np.argwhere(bad)[0])}"


# ---- one launch of every kind ------------------------------------------------------------------------------------------------------------
def _plain(dev, form, p, red, q, pad, Pd, Qd, what, S=1):
    from mindrec_amd import ops
    M, K, N = T.mkn(form, p, red, q)
    if form == 2:
        buf, win = _slab_window(S, p, q, pad, dev)
        ops.x3_gemm(2, Pd, Qd, M, K, N, win, S=S)
        return _read(buf, S * p, q, what).reshape(S, p, q)
    buf, win = _window(p, q, pad, dev)
    ops.x3_gemm(form, Pd, Qd, M, K, N, win)
    return _read(buf, p, q, what)


def _fused_fwd(dev, p, red, q, pad, Pd, Qd, plain, what, relu=True, drop=None):
    """x3_fwd: bias + ReLU + parts in the epilogue == the host's fp32 bias + ReLU of the plain product; -> (device output, host output)"""
    from mindrec_amd import ops
    b = np.random.default_rng(q).standard_normal(q).astype(np.float32)
    buf, win = _window(p, q, pad, dev)
    img = ops.x3_parts(p, q, dev)
    ops.x3_fwd(Pd, Qd, p, red, q, win, bias=torch.from_numpy(b).to(dev), relu=relu, parts_out=img, drop_next=drop)
    y = _read(buf, p, q, what)
    if drop is None:
        want = plain + b[None, :]
        want = np.maximum(want, np.float32(0)) if relu else want
        assert want.dtype == np.float32 and np.array_equal(y, want), f"{what}: {int((y != want).sum())} elements differ from the host's bias + ReLU of the plain product"
    _check_parts(img, y, what)
    return win, y


def _fused_dgrad(dev, p, red, q, pad, Pd, Qd, plain, what, scale=1.25):
    """x3_dgrad with h, scale, colsum, parts == the host's (h > 0 ? plain : 0) * scale; column sums against the output's own"""
    from mindrec_amd import ops
    h = np.random.default_rng(p + q).standard_normal((p, q)).astype(np.float32)
    hbuf = torch.full((p + 2, q + pad), NAN, dtype=torch.float32, device=dev)      # the mask source in a window of the same stride
    hbuf[:p, :q] = torch.from_numpy(h).to(dev)
    buf, win = _window(p, q, pad, dev)
    cbuf, cs = _guarded((-(-p // 64), q), dev)
    img = ops.x3_parts(p, q, dev)
    ops.x3_dgrad(Pd, Qd, p, q, red, win, h=hbuf[:p, :q], scale=scale, colsum=cs, parts_out=img)
    dx = _read(buf, p, q, what)
    want = np.where(h > 0, plain, np.float32(0)) * np.float32(scale)
    assert want.dtype == np.float32 and np.array_equal(dx, want), f"{what}: {int((dx != want).sum())} elements differ from the host's mask . scale of the plain product"
    _check_colsum(_read_guarded(cbuf, cs, what + " colsum"), dx, what)
    _check_parts(img, dx, what)


# ---- 0. the simplest exact case decides whether the MFMA adds integers below 2^24 exactly ------------------------------------------------
@pytest.mark.parametrize("family", T.FAMILIES)
def test_simplest_exact_case(dev, family):
    """one interior 128 x 256 tile, one K-tile per segment"""
    from mindrec_amd import ops
    form, p, red, q = T.SIMPLEST
    T.require_rows(ops, form, *T.mkn(form, p, red, q), 128)
    A, B = T.exact_inputs(family, form, p, red, q)
    Pd, Qd = _images(form, A, B, dev)
    what = f"form {form} {p} x {red} x {q}"
    _check(family, _plain(dev, form, p, red, q, 8, Pd, Qd, what), A, B, what)


# ---- 1. 128-row tiles: one extent at a time around the base ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("extent", ["red", "p", "q"])
def test_128_row_sweep(dev, form, extent):
    from mindrec_amd import ops
    p0, r0, q0 = T.BASE
    cases = {"red": [(p0, r, q0) for r in T.SWEEP_RED], "p": [(p, r0, q0) for p in T.SWEEP_P], "q": [(p0, r0, q) for q in T.SWEEP_Q]}[extent]
    seen = set()
    for p, red, q in cases:
        M, K, N = T.mkn(form, p, red, q)
        T.require_rows(ops, form, M, K, N, 128)
        e32 = None
        for kind in INPUTS:
            A, B = _inputs(kind, form, p, red, q)
            Pd, Qd = _images(form, A, B, dev)
            if form == 2 and kind == "general":
                e32 = _e32(A, B, dev)
            for pad in T.PADS:
                what = f"form {form} (M, K, N) = ({M}, {K}, {N}) pad {pad} {kind}"
                seen.add((q % 4, (q + pad) % 4))
                out = _plain(dev, form, p, red, q, pad, Pd, Qd, what)
                if form == 2:
                    _check_slab_sum(kind, out, A, B, e32, what)
                else:
                    _check(kind, out, A, B, what)
                if form == 0 and kind in ("general", "p"):
                    _fused_fwd(dev, p, red, q, pad, Pd, Qd, out, what + " x3_fwd", relu=pad == 8 or kind == "general")
                if form == 1 and kind in ("general", "q"):
                    _fused_dgrad(dev, p, red, q, pad, Pd, Qd, out, what + " x3_dgrad", scale=1.25 if kind == "general" else 1.0)
    assert seen == ({(0, 0), (0, 2), (2, 0), (2, 2)} if extent == "q" else {(2, 0), (2, 2)})


# ---- 2. form 2: every slab split ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", T.SLAB_M)
@pytest.mark.parametrize("K,N", T.SLAB_KN)
def test_form2_slab_splits(dev, M, K, N):
    from mindrec_amd import _lib, ops
    Tt = 6 * (T.up64(M) // 64)
    ok, refused = T.slab_counts(Tt)
    pad = 6 if (M + K) % 4 < 2 else 8
    for kind in INPUTS:
        A, B = _inputs(kind, 2, K, M, N)
        Pd, Qd = _images(2, A, B, dev)
        e32 = _e32(A, B, dev) if kind == "general" else None
        done = {}
        for s in range(1, Tt + 1):
            S = ops.x3_slabs(M, s)
            assert S in ok and S <= s
            if S in done:
                continue
            T.require_rows(ops, 2, M, K, N, 128, S)
            what = f"form 2 (M, K, N) = ({M}, {K}, {N}) S = {S} {kind}"
            done[S] = _plain(dev, 2, K, M, N, pad, Pd, Qd, what, S=S)           # (every slab fully written: _read)
            _check_slab_sum(kind, done[S], A, B, e32, what)
        assert sorted(done) == ok
        if kind == "general":
            for S in refused:
                buf, win = _slab_window(S, K, N, pad, dev)
                with pytest.raises(_lib.MrecError) as e:
                    ops.x3_gemm(2, Pd, Qd, M, K, N, win, S=S)
                assert e.value.code == -1 and bool(torch.isnan(buf).all()), f"refused S = {S}: output touched"


# ---- 3. 256-row tiles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("case", range(len(T.MR8_GEMM)), ids=[c[0] for c in T.MR8_GEMM])
def test_256_row_tiles(dev, case, kind):
    from mindrec_amd import ops
    name, form, (M, K, N), S = T.MR8_GEMM[case]
    T.require_rows(ops, form, M, K, N, 256, S)
    p, red, q = {0: (M, K, N), 1: (M, N, K), 2: (K, M, N)}[form]
    pad = 6 if kind in ("general", "p") else 8
    what = f"{name} form {form} (M, K, N) = ({M}, {K}, {N}) S = {S} pad {pad} {kind}"
    A, B = _inputs(kind, form, p, red, q)
    Pd, Qd = _images(form, A, B, dev)
    out = _plain(dev, form, p, red, q, pad, Pd, Qd, what, S=S)
    if form == 2:
        _check_slab_sum(kind, out, A, B, _e32(A, B, dev) if kind == "general" else None, what)
    else:
        _check(kind, out, A, B, what)


@pytest.mark.parametrize("pad", T.PADS)
def test_256_row_fused_forward(dev, pad):
    """bias + ReLU + parts at (3969, 66, 2050): the last tile column holds 2 columns"""
    from mindrec_amd import ops
    M, K, N = T.MR8_FWD
    T.require_rows(ops, 0, M, K, N, 256)
    A, B = T.general_inputs(0, M, K, N)
    Pd, Qd = _images(0, A, B, dev)
    what = f"x3_fwd (M, K, N) = ({M}, {K}, {N}) pad {pad}"
    plain = _plain(dev, 0, M, K, N, pad, Pd, Qd, what + " plain")
    _check("general", plain, A, B, what)
    _fused_fwd(dev, M, K, N, pad, Pd, Qd, plain, what)


def test_256_row_fused_forward_with_dropout(dev):
    """... and its neighbour N = 2052 with drop_next: == bias + ReLU, then ops.dropout_ on the undropped output, then the split"""
    from mindrec_amd import ops
    M, K, N = T.MR8_FWD_DROP
    T.require_rows(ops, 0, M, K, N, 256)
    A, B = T.general_inputs(0, M, K, N)
    Pd, Qd = _images(0, A, B, dev)
    what = f"x3_fwd (M, K, N) = ({M}, {K}, {N}) drop_next"
    plain = _plain(dev, 0, M, K, N, 6, Pd, Qd, what + " plain")
    _check("general", plain, A, B, what)
    undropped, _ = _fused_fwd(dev, M, K, N, 6, Pd, Qd, plain, what + " undropped")
    drop = ops.Dropout(0.8, seed=77, layer=2, step=5, row0=1000)
    dropped, y = _fused_fwd(dev, M, K, N, 6, Pd, Qd, plain, what, drop=drop)
    want = ops.dropout_(undropped.contiguous(), drop)
    assert torch.equal(dropped.contiguous(), want), f"{what}: differs from ops.dropout_ on the undropped output"
    assert 0.1 < float((y == 0).mean()) < 0.95


@pytest.mark.parametrize("pad", T.PADS)
def test_256_row_fused_input_gradient(dev, pad):
    """h, scale = 1.25, colsum [63, 2050], parts at (3969, 2050, 66): the last 64-row group holds one row, the fourth group of the
    last tile is empty"""
    from mindrec_amd import ops
    M, K, N = T.MR8_DGRAD
    T.require_rows(ops, 1, M, K, N, 256)
    assert -(-M // 64) == 63 and M % 64 == 1 and M % 256 == 129
    A, B = T.general_inputs(1, M, N, K)
    Pd, Qd = _images(1, A, B, dev)
    what = f"x3_dgrad (M, K, N) = ({M}, {K}, {N}) pad {pad}"
    plain = _plain(dev, 1, M, N, K, pad, Pd, Qd, what + " plain")
    _check("general", plain, A, B, what)
    _fused_dgrad(dev, M, N, K, pad, Pd, Qd, plain, what)


# ---- 4. the split input gradient (k_x3_pair + k_x3_fold_cols) ---------------------------------------------------------------------------------
def _split_dgrad(dev, M, K, N, S, rem, kind, pad, what):
    from mindrec_amd import _lib, ops
    T.require_split(_lib, M, K, N, S, rem)
    A, B = _inputs(kind, 1, M, N, K)
    Pd, Qd = _images(1, A, B, dev)
    if pad:
        buf, win = _window(M, K, pad, dev)
    else:                                                   # row stride K
        buf = torch.full((M + 2, K), NAN, dtype=torch.float32, device=dev)
        win = buf[:M]
    ops.x3_dgrad(Pd, Qd, M, K, N, win)
    dx = _read(buf, M, K, what)
    _check(kind, dx, A, B, what)
    c0 = T.split_plan(M, K, N)[1] if S else K
    one = ops.x3_gemm(1, Pd, Qd, M, K, N, torch.empty((M, K), dtype=torch.float32, device=dev)).cpu().numpy()
    assert np.array_equal(dx[:, :c0], one[:, :c0]), f"{what}: the columns left of {c0} differ from the one-launch form"


@pytest.mark.parametrize("case", range(len(T.SPLIT_TAKEN)), ids=[f"rem{c[2]}" for c in T.SPLIT_TAKEN])
def test_split_input_gradient(dev, case):
    (M, K, N), S, rem = T.SPLIT_TAKEN[case]
    assert K % 4 == 2
    _split_dgrad(dev, M, K, N, S, rem, "general", 0, f"split x3_dgrad (M, K, N) = ({M}, {K}, {N}) S = {S} rem = {rem}")


def test_split_input_gradient_exact(dev):
    (M, K, N), S, rem = T.SPLIT_TAKEN[0]
    _split_dgrad(dev, M, K, N, S, rem, "p", 0, f"split x3_dgrad (M, K, N) = ({M}, {K}, {N}) exact")


def test_split_input_gradient_in_a_16_byte_strided_window(dev):
    (M, K, N), S, rem = T.SPLIT_TAKEN[1]
    assert (K + 6) % 4 == 0
    _split_dgrad(dev, M, K, N, S, rem, "general", 6, f"split x3_dgrad (M, K, N) = ({M}, {K}, {N}) ld = {K + 6}")


def test_split_input_gradient_not_taken_at_224_columns(dev):
    M, K, N = T.SPLIT_NOT_TAKEN
    _split_dgrad(dev, M, K, N, 0, 0, "general", 0, f"one-launch x3_dgrad (M, K, N) = ({M}, {K}, {N})")


# ---- 5. the post kernels (k_x3_post modes 0, 1, 2) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", T.POST_R)
def test_post_kernels(dev, R):
    from mindrec_amd import ops
    for C in T.POST_C:
        for extra in (0, 2):
            what = f"R = {R} C = {C} ld = {C + extra}"
            rng = np.random.default_rng(R * 4096 + C + extra)
            acc = rng.standard_normal((R, C)).astype(np.float32)
            b = rng.standard_normal(C).astype(np.float32)
            h = rng.standard_normal((R, C)).astype(np.float32)

            def window():
                buf = torch.full((R + 2, C + extra), NAN, dtype=torch.float32, device=dev)
                buf[:R, :C] = torch.from_numpy(acc).to(dev)
                return buf, buf[:R, :C]
            # mode 0: the split alone, into an image that holds ones: the padding is the kernel's to zero
            buf, win = window()
            img = torch.ones((3, T.up64(R), T.up64(C)), dtype=torch.bfloat16, device=dev)
            ops.x3_split(win, out=img)
            assert np.array_equal(_read(buf, R, C, what + " split"), acc)
            _check_parts(img, acc, what + " split")
            # mode 1: bias + ReLU in place, parts
            for relu in (True, False):
                buf, win = window()
                img = ops.x3_parts(R, C, dev)
                ops.x3_bias_relu_(win, torch.from_numpy(b).to(dev), relu=relu, parts_out=img)
                y = _read(buf, R, C, what + " bias_relu")
                want = np.maximum(acc + b, np.float32(0)) if relu else acc + b
                assert np.array_equal(y, want), what + " bias_relu"
                _check_parts(img, y, what + " bias_relu")
            # mode 2: ReLU mask, scale, column sums per 64 rows (the last block partly filled), parts
            for scale in (1.0, 1.25):
                buf, win = window()
                img = ops.x3_parts(R, C, dev)
                cbuf, cs = _guarded((-(-R // 64), C), dev)
                ops.x3_mask_colsum_(win, torch.from_numpy(h).to(dev), cs, img, scale=scale)
                dx = _read(buf, R, C, what + " mask_colsum")
                want = np.where(h > 0, acc, np.float32(0)) * np.float32(scale)
                assert np.array_equal(dx, want), what + " mask_colsum"
                sums = _read_guarded(cbuf, cs, what + " colsum")
                for g in range(sums.shape[0]):
                    assert np.allclose(sums[g], dx[g * 64:(g + 1) * 64].astype(np.float64).sum(0), rtol=1e-5, atol=1e-5), f"{what}: column sums of block {g}"
                _check_parts(img, dx, what + " mask_colsum")
    assert R % 64 != 0
