"""Every conv and head kernel against an fp64 CPU reference, bit for bit.

Operands are small integers (tests/helpers.py: rounding, wide-significand and statistics regimes), scales are powers of two, shifts
half-integers: every product and every partial sum is exact in fp32 whatever the order, tile, split, ring or reduce pass, so an fp32
kernel must reproduce the reference exactly and a bf16 kernel its round-to-nearest-even.  The tolerance is zero and derived; a truncating
store, a double rounding, a dropped or doubled product at a border, a wrong epilogue order or a skipped partial all change bits here while
they pass the Gaussian tolerance tests.  tests/test_exact_cases_cpu.py checks the conditions on the inputs (asserted again here before
every comparison) and that the cases reach every kernel of the dispatch plan; each test asserts the kernel its case is meant to reach.

Tensors whose raw pointers go to the C ABI are named locals that outlive the launch; every output buffer is NaN-filled first."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import helpers as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32
REGIMES = ("round", "wide_a", "wide_b")


def to_nhwc(t, dt=F32):      # (B, C, H, W) cpu -> (B, H, W, C) device
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).to(dt)


def nan_out(shape, dt=F32):
    return torch.full(tuple(shape), NAN, dtype=dt, device=DEV)


def expect_nhwc(ref64, bf16):
    """fp64 NCHW reference -> the fp32 values the kernel must store (bf16: nearest-even), as NHWC so that a mismatch reads (b, y, x, channel)"""
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64)
    return (X.bf16_rne(ref32) if bf16 else ref32).permute(0, 2, 3, 1).contiguous()


def same(got_nhwc, ref64, bf16, what):
    assert got_nhwc.dtype == (BF16 if bf16 else F32)
    X.assert_equal_report(got_nhwc.float(), expect_nhwc(ref64, bf16), what)


def lib_and_desc(geom):
    from structuredetector_amd import _lib as L
    return L, L.lib(), X.conv_desc(L, geom)


def kname(lib, d, p):
    return lib.sd_conv2d_kernel_name(C.byref(d), p).decode()


def entries(p):
    return [e for e in X.EXACT_CONV_CASES if p in e[2]]


def regimes_of(geom):
    return ("round",) if geom == X.BIG_TILE_CASE or X.conv_macs(geom) > 2 ** 30 else REGIMES


def krsc_t(w, dt=F32):       # (Cout, Cin, k, k) -> data-gradient layout [Cin][R][S][Cout]
    return w.permute(1, 2, 3, 0).contiguous().to(DEV).to(dt)


def upsample2(t):
    return F.interpolate(t, scale_factor=2, mode="nearest")


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def forward_variants(geom, p, regime, Ho, Wo):
    """(tag, scale, shift, residual, res_up2, relu, fp64 reference): plain, the full epilogue, the half-size residual of the FPN laterals"""
    cout = geom[4]
    scale, shift, res = X.epilogue_operands(geom, cout, p["ref"].shape, wide=regime != "round")
    out = [("plain", None, None, None, 0, 0, p["ref"]),
           ("scale+shift+residual+relu", scale, shift, res, 0, 1, X.epilogue_ref(p["ref"], scale, shift, res, True)),
           ("scale+shift+relu", scale, shift, None, 0, 1, X.epilogue_ref(p["ref"], scale, shift, None, True))]
    X.assert_exact_reference(out[1][6], X.epilogue_bound(p["bound"], scale, shift, res), X.EXACT_LIMIT_HALVES, "epilogue")
    if X.conv_macs(geom) > 2 ** 30:          # the two largest cases: plain and the full epilogue
        return out[:2]
    if Ho % 2 == 0 and Wo % 2 == 0:
        half = res[:, :, :Ho // 2, :Wo // 2].contiguous()
        out.append(("shift+res_up2", None, shift, half, 1, 0, X.epilogue_ref(p["ref"], None, shift, upsample2(half), False)))
    return out


def run_forward(entry, bf16):
    geom, opts, names = entry
    L, lib, d = lib_and_desc(geom)
    dt = BF16 if bf16 else F32
    fwd = lib.sd_conv2d_fwd_bf16 if bf16 else lib.sd_conv2d_fwd
    with X.dispatch_options(lib, opts):
        assert kname(lib, d, 16 if bf16 else 0) == names[16 if bf16 else 0]
        nws = (lib.sd_conv2d_fwd_bf16_workspace_bytes if bf16 else lib.sd_conv2d_fwd_workspace_bytes)(C.byref(d))
        if opts.get("conv_fwd_split_k", 1) == 0:
            assert nws == 0
        ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
        for regime in (("round",) if bf16 else regimes_of(geom)):
            p = X.fwd_problem(geom, regime)
            ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"{geom} {regime}")
            if bf16:
                print(geom, "rounding shares", X.assert_rounding_coverage(ref32, str(geom)))
            xd, wd = to_nhwc(p["x"], dt), to_nhwc(p["w"], dt)
            for tag, scale, shift, res, up2, relu, ref in forward_variants(geom, p, regime, d.Ho, d.Wo):
                sc = scale.to(DEV) if scale is not None else None
                sh = shift.to(DEV) if shift is not None else None
                rd = to_nhwc(res, dt) if res is not None else None
                for with_ws in ((True, False) if nws else (False,)):      # split-K + reduce pass, and the single-pass kernel
                    y = nan_out((geom[0], d.Ho, d.Wo, geom[4]), dt)
                    L.check(fwd(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), C.byref(d), sc.data_ptr() if sc is not None else 0,
                                sh.data_ptr() if sh is not None else 0, rd.data_ptr() if rd is not None else 0, up2, relu,
                                ws.data_ptr() if with_ws else 0, nws if with_ws else 0, L.stream()))
                    same(y, ref, bf16, f"{geom} {opts} {regime} {tag} workspace={with_ws}")


@pytest.mark.parametrize("entry", entries(0), ids=X.case_id)
def test_conv_fwd_f32(entry):
    """sd_conv2d_fwd: plain, scale + shift + residual + ReLU, res_up2; with the workspace (split-K and its reduce pass, where the plan splits)
    and without (single pass); rounding regime and both wide-significand roles (an fp32 path that narrows an operand changes bits)."""
    run_forward(entry, False)


@pytest.mark.parametrize("entry", entries(16), ids=X.case_id)
def test_conv_fwd_bf16(entry):
    """sd_conv2d_fwd_bf16 with every epilogue form: the stored bf16 value is the nearest-even rounding of the exact result, once."""
    run_forward(entry, True)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("geom", X.EXACT_SB_CASES, ids=lambda g: "x".join(map(str, g)))
def test_conv_fwd_small_batch_kernel(geom, bf16):
    """sd_conv2d_fwd_sb: the partial tiles of every K slice are combined inside the launch; two calls back to back through the same
    workspace and ticket state (left zero), plain and with the epilogue (x2-upsampled residual for the 1x1 laterals)."""
    L, lib, d = lib_and_desc(geom)
    dt = BF16 if bf16 else F32
    assert lib.sd_conv2d_fwd_sb_supported(C.byref(d), bf16) in (0, 1)
    nws, nst = lib.sd_conv2d_fwd_sb_workspace_bytes(C.byref(d), bf16), lib.sd_conv2d_fwd_sb_state_bytes(C.byref(d), bf16)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    st = torch.zeros(max(nst, 256), dtype=torch.uint8, device=DEV)
    for regime in (("round",) if bf16 else REGIMES):
        p = X.fwd_problem(geom, regime)
        X.assert_exact_reference(p["ref"], p["bound"], what=f"{geom} {regime}")
        xd, wd = to_nhwc(p["x"], dt), to_nhwc(p["w"], dt)
        variants = forward_variants(geom, p, regime, d.Ho, d.Wo)
        outs = []
        for tag, scale, shift, res, up2, relu, ref in variants:
            sc = scale.to(DEV) if scale is not None else None
            sh = shift.to(DEV) if shift is not None else None
            rd = to_nhwc(res, dt) if res is not None else None
            y = nan_out((geom[0], d.Ho, d.Wo, geom[4]), dt)
            L.check(lib.sd_conv2d_fwd_sb(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), C.byref(d), sc.data_ptr() if sc is not None else 0,
                                         sh.data_ptr() if sh is not None else 0, rd.data_ptr() if rd is not None else 0, up2, relu, bf16,
                                         ws.data_ptr(), ws.numel(), st.data_ptr(), st.numel(), L.stream()))
            outs.append((y, ref, tag, sc, sh, rd))                 # launched back to back; compared after the last one
        for y, ref, tag, *_ in outs:
            same(y, ref, bool(bf16), f"sb {geom} {regime} {tag}")
    assert int(st.view(torch.int32).abs().sum()) == 0, "arrival tickets must be left zero"


# ---- data gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", entries(1), ids=X.case_id)
def test_conv_dgrad_f32(entry):
    """sd_conv2d_transpose_weights (a pure permutation) + sd_conv2d_dgrad plain and + residual + sd_conv2d_dgrad_half_res: unit stride,
    stride-2 parity classes, generic strided, strided 1x1."""
    geom, opts, names = entry
    B, H, W, cin, cout, k, stride, pad = geom
    L, lib, d = lib_and_desc(geom)
    with X.dispatch_options(lib, opts):
        assert kname(lib, d, 1) == names[1]
        for regime in regimes_of(geom):
            p = X.dgrad_problem(geom, regime)
            X.assert_exact_reference(p["ref"], p["bound"], what=f"{geom} {regime}")
            _, _, res = X.epilogue_operands(geom, cin, p["ref"].shape, salt=1, wide=regime != "round")
            X.assert_exact_reference(p["ref"] + res.double(), p["bound"] + res.double().abs(), what="dgrad + residual")
            dyd, wd = to_nhwc(p["dy"]), to_nhwc(p["w"])
            wt = nan_out((cin, k, k, cout))
            L.check(lib.sd_conv2d_transpose_weights(wd.data_ptr(), wt.data_ptr(), cout, k * k, cin, L.stream()))
            X.assert_equal_report(wt, p["w"].permute(1, 2, 3, 0).contiguous(), f"transpose {geom}", "ci, r, s, co")
            dx = nan_out((B, H, W, cin))
            L.check(lib.sd_conv2d_dgrad(dyd.data_ptr(), wt.data_ptr(), dx.data_ptr(), C.byref(d), 0, L.stream()))
            same(dx, p["ref"], False, f"dgrad {geom} {opts} {regime}")
            resd = to_nhwc(res)
            dx2 = nan_out((B, H, W, cin))
            L.check(lib.sd_conv2d_dgrad(dyd.data_ptr(), wt.data_ptr(), dx2.data_ptr(), C.byref(d), resd.data_ptr(), L.stream()))
            same(dx2, p["ref"] + res.double(), False, f"dgrad + residual {geom} {opts} {regime}")
            if H % 2 == 0 and W % 2 == 0:
                half = res[:, :, :H // 2, :W // 2].contiguous()
                full = torch.zeros_like(res)
                full[:, :, ::2, ::2] = half
                halfd = to_nhwc(half)
                dx3 = nan_out((B, H, W, cin))
                L.check(lib.sd_conv2d_dgrad_half_res(dyd.data_ptr(), wt.data_ptr(), dx3.data_ptr(), C.byref(d), halfd.data_ptr(), L.stream()))
                same(dx3, p["ref"] + full.double(), False, f"dgrad + half-size residual {geom} {opts} {regime}")


@pytest.mark.parametrize("entry", entries(17), ids=X.case_id)
def test_conv_dgrad_bf16(entry):
    """sd_conv2d_transpose_weights_bf16 + sd_conv2d_dgrad_bf16 with residual modes 0 / 1 / 2."""
    geom, opts, names = entry
    B, H, W, cin, cout, k, stride, pad = geom
    L, lib, d = lib_and_desc(geom)
    with X.dispatch_options(lib, opts):
        assert kname(lib, d, 17) == names[17]
        p = X.dgrad_problem(geom, "round")
        ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=str(geom))
        X.assert_rounding_coverage(ref32[:, :, ::2, ::2] if k == 1 and stride == 2 else ref32, str(geom))
        _, _, res = X.epilogue_operands(geom, cin, p["ref"].shape, salt=1)
        dyd, wd = to_nhwc(p["dy"], BF16), to_nhwc(p["w"])
        wt = nan_out((cin, k, k, cout), BF16)
        L.check(lib.sd_conv2d_transpose_weights_bf16(wd.data_ptr(), wt.data_ptr(), cout, k * k, cin, L.stream()))
        X.assert_equal_report(wt.float(), p["w"].permute(1, 2, 3, 0).contiguous(), f"transpose bf16 {geom}", "ci, r, s, co")
        resd = to_nhwc(res, BF16)
        modes = [(0, None, p["ref"]), (1, resd, p["ref"] + res.double())]
        if H % 2 == 0 and W % 2 == 0:
            half = res[:, :, :H // 2, :W // 2].contiguous()
            full = torch.zeros_like(res)
            full[:, :, ::2, ::2] = half
            modes.append((2, to_nhwc(half, BF16), p["ref"] + full.double()))
        for mode, r, ref in modes:
            dx = nan_out((B, H, W, cin), BF16)
            L.check(lib.sd_conv2d_dgrad_bf16(dyd.data_ptr(), wt.data_ptr(), dx.data_ptr(), C.byref(d), r.data_ptr() if r is not None else 0, mode, L.stream()))
            same(dx, ref, True, f"dgrad bf16 {geom} {opts} residual mode {mode}")


# ---- weight gradient -----------------------------------------------------------------------------------------------------------------
def run_wgrad(geom, bf16, what):
    B, H, W, cin, cout, k, stride, pad = geom
    L, lib, d = lib_and_desc(geom)
    dt = BF16 if bf16 else F32
    fn = lib.sd_conv2d_wgrad_bf16 if bf16 else lib.sd_conv2d_wgrad
    nws = (lib.sd_conv2d_wgrad_bf16_workspace_bytes if bf16 else lib.sd_conv2d_wgrad_workspace_bytes)(C.byref(d))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    for regime in (("round",) if bf16 else REGIMES):
        p = X.wgrad_problem(geom, regime)
        X.assert_exact_reference(p["ref"], p["bound"], what=f"{geom} {regime}")
        base = X.int_uniform(torch.Generator().manual_seed(5), p["ref"].shape, 2047)
        X.assert_exact_reference(p["ref"] + base.double(), p["bound"] + base.double().abs(), what="accumulate")
        dyd, xd = to_nhwc(p["dy"], dt), to_nhwc(p["x"], dt)
        dw = nan_out((cout, k, k, cin))
        ws.fill_(0xFF)                       # (NaNs: a partial the kernel does not write must not be summed)
        L.check(fn(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), C.byref(d), 0, ws.data_ptr(), ws.numel(), L.stream()))
        X.assert_equal_report(dw, p["ref"].float().permute(0, 2, 3, 1).contiguous(), f"{what} {regime}", "co, r, s, ci")
        acc = to_nhwc(base)
        L.check(fn(dyd.data_ptr(), xd.data_ptr(), acc.data_ptr(), C.byref(d), 1, ws.data_ptr(), ws.numel(), L.stream()))
        X.assert_equal_report(acc, (p["ref"] + base.double()).float().permute(0, 2, 3, 1).contiguous(), f"{what} {regime} accumulate", "co, r, s, ci")


@pytest.mark.parametrize("entry", entries(2), ids=X.case_id)
def test_conv_wgrad_f32(entry):
    """sd_conv2d_wgrad: tile kernels, the all-taps forms (wgrad_f32_ring 0 / 1 / 2, 16-wide maps) and their reduce passes; accumulate 0
    and 1 onto an integer base."""
    geom, opts, names = entry
    L, lib, d = lib_and_desc(geom)
    with X.dispatch_options(lib, opts):
        assert kname(lib, d, 2) == names[2]
        run_wgrad(geom, False, f"wgrad {geom} {opts}")


@pytest.mark.parametrize("geom", X.EXACT_WGRAD_BF16_CASES, ids=lambda g: "x".join(map(str, g)))
def test_conv_wgrad_bf16(geom):
    """sd_conv2d_wgrad_bf16 (fp32 dW from bf16 dy / x): every ring form where the geometry has one, the tap kernels and the widened path."""
    L, lib, d = lib_and_desc(geom)
    rings = X.WGRAD_BF16_RINGS if geom[5] == 3 and geom[6] == 1 and d.Wo % 32 == 0 else (5,)
    for ring in rings:
        with X.dispatch_options(lib, {"wgrad_bf16_ring": ring}):
            run_wgrad(geom, True, f"wgrad bf16 {geom} ring {ring}")


# ---- stem ------------------------------------------------------------------------------------------------------------------------------
def stem_desc(shape):
    B, H, W = shape
    return lib_and_desc((B, H, W, 3, 64, 7, 2, 3))


@pytest.mark.parametrize("shape", X.EXACT_STEM_SHAPES)
def test_stem_forward(shape):
    """sd_conv2d_stem_fwd fp32 (all regimes) and out_bf16, with and without workspace, plain and scale + shift + ReLU; and the fused
    sd_stem_bn_relu_maxpool_fwd_bf16 (power-of-two scale, integer shift: the max-pool of exact values is exact)."""
    L, lib, d = stem_desc(shape)
    B = shape[0]
    nws = lib.sd_conv2d_stem_fwd_workspace_bytes(C.byref(d))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    geom = (B, shape[1], shape[2], 3, 64, 7, 2, 3)
    for out_bf16 in (0, 1):
        for regime in (("round",) if out_bf16 else REGIMES):
            p = X.stem_problem(shape, regime)
            ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"stem {shape} {regime}")
            if out_bf16:
                X.assert_rounding_coverage(ref32, f"stem {shape}")
            scale, shift, _ = X.epilogue_operands(geom, 64, (1,))
            full = X.epilogue_ref(p["ref"], scale, shift, None, True)
            X.assert_exact_reference(full, X.epilogue_bound(p["bound"], scale, shift), X.EXACT_LIMIT_HALVES, "stem epilogue")
            xd, wd, sc, sh = p["x"].to(DEV), to_nhwc(p["w"]), scale.to(DEV), shift.to(DEV)
            for with_ws in ((True,) if out_bf16 else (True, False)):       # (the bf16 output has no generic no-workspace kernel)
                for tag, s_, h_, relu, ref in (("plain", 0, 0, 0, p["ref"]), ("scale+shift+relu", sc.data_ptr(), sh.data_ptr(), 1, full)):
                    y = nan_out((B, d.Ho, d.Wo, 64), BF16 if out_bf16 else F32)
                    L.check(lib.sd_conv2d_stem_fwd(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), C.byref(d), s_, h_, relu, out_bf16,
                                                   ws.data_ptr() if with_ws else 0, nws if with_ws else 0, L.stream()))
                    same(y, ref, bool(out_bf16), f"stem {shape} {regime} {tag} bf16={out_bf16} workspace={with_ws}")
    # conv -> folded BatchNorm -> ReLU -> MaxPool(3, 2, 1) in one launch, bf16 pooled output
    p = X.stem_problem(shape, "round")
    g = torch.Generator().manual_seed(sum(shape))
    scale, shift = X.pow2_scales(g, 64), X.int_uniform(g, (64,), 32)
    act = X.epilogue_ref(p["ref"], scale, shift, None, True)
    X.assert_exact_reference(act, X.epilogue_bound(p["bound"], scale, shift), what="stem + pool")
    pooled = F.max_pool2d(X.bf16_rne(act.float()), 3, 2, 1)           # (rounding is monotonic: max of rounded = rounded max)
    xd, wd, sc, sh = p["x"].to(DEV), to_nhwc(p["w"]), scale.to(DEV), shift.to(DEV)
    yp = nan_out((B, d.Ho // 2, d.Wo // 2, 64), BF16)
    L.check(lib.sd_stem_bn_relu_maxpool_fwd_bf16(xd.data_ptr(), wd.data_ptr(), sc.data_ptr(), sh.data_ptr(), yp.data_ptr(), C.byref(d), L.stream()))
    X.assert_equal_report(yp.float(), pooled.permute(0, 2, 3, 1).contiguous(), f"stem + pool {shape}")


@pytest.mark.parametrize("shape", X.EXACT_STEM_SHAPES)
def test_stem_weight_gradient(shape):
    """sd_conv2d_stem_wgrad (fp32, all regimes), _bf16mm (operands rounded to bf16 on the way in) and _bf16 (bf16 dy): accumulate 0 and 1."""
    L, lib, d = stem_desc(shape)
    geom = (shape[0], shape[1], shape[2], 3, 64, 7, 2, 3)
    nws = lib.sd_conv2d_stem_wgrad_workspace_bytes(C.byref(d))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    for name, fn, dy_dt, regimes in (("f32", lib.sd_conv2d_stem_wgrad, F32, REGIMES), ("bf16mm", lib.sd_conv2d_stem_wgrad_bf16mm, F32, ("round",)),
                                     ("bf16", lib.sd_conv2d_stem_wgrad_bf16, BF16, ("round",))):
        for regime in regimes:
            p = X.wgrad_problem(geom, regime)
            X.assert_exact_reference(p["ref"], p["bound"], what=f"stem wgrad {shape} {regime}")
            base = X.int_uniform(torch.Generator().manual_seed(6), p["ref"].shape, 2047)
            X.assert_exact_reference(p["ref"] + base.double(), p["bound"] + base.double().abs(), what="accumulate")
            dyd, xd = to_nhwc(p["dy"], dy_dt), p["x"].to(DEV)
            dw = nan_out((64, 7, 7, 3))
            ws.fill_(0xFF)
            L.check(fn(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), C.byref(d), 0, ws.data_ptr(), ws.numel(), L.stream()))
            X.assert_equal_report(dw, p["ref"].float().permute(0, 2, 3, 1).contiguous(), f"stem wgrad {name} {shape} {regime}", "co, r, s, ci")
            acc = to_nhwc(base)
            L.check(fn(dyd.data_ptr(), xd.data_ptr(), acc.data_ptr(), C.byref(d), 1, ws.data_ptr(), ws.numel(), L.stream()))
            X.assert_equal_report(acc, (p["ref"] + base.double()).float().permute(0, 2, 3, 1).contiguous(), f"stem wgrad {name} {shape} {regime} accumulate",
                                  "co, r, s, ci")


# ---- statistics regime: the entry points that return raw sums ----------------------------------------------------------------------------
def check_sums(sums, y_stored64, what):
    """sums == [sum y (C), sum y^2 (C), M] exactly, y = the stored output as fp64 NCHW"""
    Cc = y_stored64.shape[1]
    assert float((y_stored64 ** 2).sum((0, 2, 3)).max()) < X.EXACT_LIMIT, "sum of squares bound"
    want = torch.cat([y_stored64.sum((0, 2, 3)), (y_stored64 ** 2).sum((0, 2, 3)), torch.tensor([y_stored64.numel() / Cc], dtype=torch.float64)])
    X.assert_equal_report(sums, want, what, "index into [S0 (C), S1 (C), n]")


@pytest.mark.parametrize("entry", X.EXACT_STATS_CASES, ids=X.case_id)
def test_conv_fwd_bn_sums(entry):
    """sd_conv2d_fwd_bn_sums / sd_conv2d_fwd_bf16_bn_sums: y exact, sums == [sum y, sum y^2, M] of the STORED y (the rounded one for bf16)."""
    geom, opts, names = entry
    L, lib, d = lib_and_desc(geom)
    p = X.fwd_problem(geom, "stats")
    ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"stats {geom}")
    with X.dispatch_options(lib, opts):
        for bf16 in (0, 1):
            if (16 if bf16 else 0) not in names:
                continue
            assert kname(lib, d, 16 if bf16 else 0) == names[16 if bf16 else 0]
            dt = BF16 if bf16 else F32
            fn = lib.sd_conv2d_fwd_bf16_bn_sums if bf16 else lib.sd_conv2d_fwd_bn_sums
            nws = (lib.sd_conv2d_fwd_bf16_bn_stats_workspace_bytes if bf16 else lib.sd_conv2d_fwd_bn_stats_workspace_bytes)(C.byref(d))
            ws = torch.full((max(nws, 256),), 0xFF, dtype=torch.uint8, device=DEV)
            xd, wd = to_nhwc(p["x"], dt), to_nhwc(p["w"], dt)
            y = nan_out((geom[0], d.Ho, d.Wo, geom[4]), dt)
            sums = torch.full((2 * geom[4] + 1,), NAN, dtype=torch.float64, device=DEV)
            L.check(fn(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), C.byref(d), sums.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()))
            same(y, p["ref"], bool(bf16), f"bn_sums y {geom} bf16={bf16}")
            check_sums(sums, (X.bf16_rne(ref32) if bf16 else ref32).double(), f"bn_sums {geom} {opts} bf16={bf16}")


@pytest.mark.parametrize("shape", X.EXACT_STEM_SHAPES)
def test_stem_fwd_bn_sums(shape):
    """sd_conv2d_stem_fwd_bn_sums, _bf16mm (fp32 y from the bf16 MFMA) and _bf16 (bf16 y, statistics of the rounded values)."""
    L, lib, d = stem_desc(shape)
    p = X.stem_problem(shape, "stats")
    ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"stem stats {shape}")
    nws = lib.sd_conv2d_stem_fwd_bn_stats_workspace_bytes(C.byref(d))
    xd, wd = p["x"].to(DEV), to_nhwc(p["w"])
    for name, fn, bf16 in (("f32", lib.sd_conv2d_stem_fwd_bn_sums, False), ("bf16mm", lib.sd_conv2d_stem_fwd_bn_sums_bf16mm, False),
                           ("bf16", lib.sd_conv2d_stem_fwd_bn_sums_bf16, True)):
        ws = torch.full((max(nws, 256),), 0xFF, dtype=torch.uint8, device=DEV)
        y = nan_out((shape[0], d.Ho, d.Wo, 64), BF16 if bf16 else F32)
        sums = torch.full((129,), NAN, dtype=torch.float64, device=DEV)
        L.check(fn(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), C.byref(d), sums.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()))
        same(y, p["ref"], bf16, f"stem bn_sums y {name} {shape}")
        check_sums(sums, (X.bf16_rne(ref32) if bf16 else ref32).double(), f"stem bn_sums {name} {shape}")


@pytest.mark.parametrize("entry", X.EXACT_BNRED_CASES, ids=X.case_id)
def test_conv_dgrad_bn_reduce_sums(entry):
    """sd_conv2d_dgrad_bn_reduce_sums with integer mean, power-of-two invstd and integer gamma / beta: dx, sums = [sum g, sum g xhat, M]
    and dgamma / dbeta (= and +=) are exact; ReLU mask from the saved output (1), recomputed from x (2) and none (0)."""
    geom, opts, name = entry
    B, H, W, cin, cout, k, stride, pad = geom
    L, lib, d = lib_and_desc(geom)
    p = X.dgrad_problem(geom, "stats")
    X.assert_exact_reference(p["ref"], p["bound"], what=f"bn reduce {geom}")
    g = torch.Generator().manual_seed(sum(geom))
    bn_x, bn_y = X.int_uniform(g, p["ref"].shape, 4), X.int_uniform(g, p["ref"].shape, 2)
    mean, invstd = X.int_uniform(g, (cin,), 2), torch.tensor([0.5, 1.0])[torch.randint(0, 2, (cin,), generator=g)]
    gamma, beta = X.int_uniform(g, (cin,), 3), X.int_uniform(g, (cin,), 3)
    res = X.int_uniform(g, p["ref"].shape, 7)
    base_g, base_b = X.int_uniform(g, (cin,), 2047), X.int_uniform(g, (cin,), 2047)
    v = lambda t: t.double().view(1, -1, 1, 1)
    xhat = (bn_x.double() - v(mean)) * v(invstd)
    with X.dispatch_options(lib, opts):
        assert kname(lib, d, 1) == name
        nws = lib.sd_conv2d_dgrad_bn_reduce_workspace_bytes(C.byref(d))
        dyd, wt = to_nhwc(p["dy"]), krsc_t(p["w"])
        xd, yd = to_nhwc(bn_x), to_nhwc(bn_y)
        md, isd, gd, bd = mean.to(DEV), invstd.to(DEV), gamma.to(DEV), beta.to(DEV)
        for relu, r, acc in ((1, None, 0), (2, res, 1), (0, res, 0)):
            dx_ref = p["ref"] + (r.double() if r is not None else 0)
            mask = (bn_y > 0) if relu == 1 else ((xhat * v(gamma) + v(beta)) > 0 if relu == 2 else torch.ones_like(bn_y, dtype=torch.bool))
            gm = dx_ref * mask
            assert float((gm * xhat).abs().sum((0, 2, 3)).max()) < X.EXACT_LIMIT_HALVES and float(gm.abs().sum((0, 2, 3)).max()) < X.EXACT_LIMIT
            s0, s1 = gm.sum((0, 2, 3)), (gm * xhat).sum((0, 2, 3))
            rd = to_nhwc(r) if r is not None else None
            ws = torch.full((max(nws, 256),), 0xFF, dtype=torch.uint8, device=DEV)
            dx = nan_out((B, H, W, cin))
            dg = base_g.to(DEV) if acc else nan_out((cin,))
            db = base_b.to(DEV) if acc else nan_out((cin,))
            sums = torch.full((2 * cin + 1,), NAN, dtype=torch.float64, device=DEV)
            L.check(lib.sd_conv2d_dgrad_bn_reduce_sums(dyd.data_ptr(), wt.data_ptr(), dx.data_ptr(), C.byref(d), rd.data_ptr() if rd is not None else 0,
                                                       xd.data_ptr(), yd.data_ptr() if relu == 1 else 0, relu, md.data_ptr(), isd.data_ptr(), gd.data_ptr(),
                                                       bd.data_ptr(), dg.data_ptr(), db.data_ptr(), acc, sums.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()))
            same(dx, dx_ref, False, f"bn reduce dx {geom} relu={relu}")
            want = torch.cat([s0, s1, torch.tensor([float(B * H * W)], dtype=torch.float64)])
            X.assert_equal_report(sums, want, f"bn reduce sums {geom} relu={relu}", "index into [S0 (C), S1 (C), n]")
            X.assert_equal_report(dg, (s1 + (base_g.double() if acc else 0)).float(), f"dgamma {geom} relu={relu} accumulate={acc}", "channel")
            X.assert_equal_report(db, (s0 + (base_b.double() if acc else 0)).float(), f"dbeta {geom} relu={relu} accumulate={acc}", "channel")


# ---- weight transposes: pure permutations, exact on any data -------------------------------------------------------------------------------
def test_transpose_weights_batched():
    """sd_conv2d_transpose_weights_batched (fp32 and bf16 output) on three convs in one launch, Gaussian data: fp32 is a permutation, bf16 a
    permutation of the nearest-even roundings."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(11)
    convs = [(64, 9, 64), (128, 1, 64), (256, 9, 128)]          # (Cout, taps, Cin)
    ws_ = [torch.randn(co, t, ci, generator=g) for co, t, ci in convs]
    flat = torch.cat([w.flatten() for w in ws_]).to(DEV)
    rows, src, dst, blk = [], 0, 0, 0
    for co, t, ci in convs:
        nbx, nby = (ci + 31) // 32, (co + 31) // 32
        rows.append([src, dst, co, t, ci, blk, nbx, nby])
        src += co * t * ci; dst += co * t * ci; blk += nbx * nby * t
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    for out_bf16 in (0, 1):
        out = nan_out((flat.numel(),), BF16 if out_bf16 else F32)
        L.check(lib.sd_conv2d_transpose_weights_batched(flat.data_ptr(), out.data_ptr(), table.data_ptr(), len(convs), blk, out_bf16, L.stream()))
        want = torch.cat([w.permute(2, 1, 0).contiguous().flatten() for w in ws_])
        X.assert_equal_report(out.float(), X.bf16_rne(want) if out_bf16 else want, f"batched transpose bf16={out_bf16}", "flat index")


# ---- heads ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.EXACT_HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_kernels(case):
    """sd_head_fwd, sd_head_fwd_bf16 (the hi / lo bf16 split of an integer weight is exact) and sd_head_bwd with accumulate 0 and 1: the
    generic kernels, the C = 128 / Co <= 16 MFMA path (HW % 16 == 0) and the wide GEMM path (Co > 32)."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    B, H, W, Cc, Co = case
    nws = lib.sd_head_bwd_workspace_bytes(B, H * W, Cc, Co)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    for regime in REGIMES:
        p = X.head_problem(case, regime)
        for key in ("y", "dx", "dw", "db"):
            X.assert_exact_reference(p[key], p[key + "_bound"], what=f"head {case} {regime} {key}")
        xd, wd, bd, dyd = to_nhwc(p["x"]), p["w"].to(DEV), p["bias"].to(DEV), p["dy"].to(DEV)
        y = nan_out((B, Co, H, W))
        L.check(lib.sd_head_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), B, H * W, Cc, Co, L.stream()))
        X.assert_equal_report(y, p["y"].float(), f"head fwd {case} {regime}", "b, co, y, x")
        if regime != "wide_a":                                   # (x is bf16 there: 12-bit activations do not exist)
            x16 = to_nhwc(p["x"], BF16)
            y16 = nan_out((B, Co, H, W))
            L.check(lib.sd_head_fwd_bf16(x16.data_ptr(), wd.data_ptr(), bd.data_ptr(), y16.data_ptr(), B, H * W, Cc, Co, L.stream()))
            X.assert_equal_report(y16, p["y"].float(), f"head fwd bf16 {case} {regime}", "b, co, y, x")
        gw, gb = torch.Generator().manual_seed(7), torch.Generator().manual_seed(8)
        base_w, base_b = X.int_uniform(gw, (Co, Cc), 2047), X.int_uniform(gb, (Co,), 2047)
        for acc in (0, 1):
            dx = nan_out((B, H, W, Cc))
            dw = base_w.to(DEV) if acc else nan_out((Co, Cc))
            db = base_b.to(DEV) if acc else nan_out((Co,))
            L.check(lib.sd_head_bwd(dyd.data_ptr(), xd.data_ptr(), wd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), B, H * W, Cc, Co, acc,
                                    ws.data_ptr(), ws.numel(), L.stream()))
            same(dx, p["dx"], False, f"head dx {case} {regime}")
            X.assert_equal_report(dw, (p["dw"] + (base_w.double() if acc else 0)).float(), f"head dw {case} {regime} accumulate={acc}", "co, c")
            X.assert_equal_report(db, (p["db"] + (base_b.double() if acc else 0)).float(), f"head dbias {case} {regime} accumulate={acc}", "co")


@pytest.mark.parametrize("case", X.EXACT_HEAD_BF16_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_backward_bf16(case):
    """sd_head_bwd_bf16: bf16 activation in, bf16 input gradient out (nearest-even of the exact value), fp32 dw / dbias, accumulate 0 and 1."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    B, H, W, Cc, Co = case
    p = X.head_problem(case, "round")
    for key in ("dx", "dw", "db"):
        X.assert_exact_reference(p[key], p[key + "_bound"], what=f"head {case} {key}")
    X.assert_rounding_coverage(p["dx"].float(), f"head dx {case}")
    ws = torch.empty(max(lib.sd_head_bwd_workspace_bytes(B, H * W, Cc, Co), 256), dtype=torch.uint8, device=DEV)
    x16, wd, dyd = to_nhwc(p["x"], BF16), p["w"].to(DEV), p["dy"].to(DEV)
    base_w, base_b = X.int_uniform(torch.Generator().manual_seed(7), (Co, Cc), 2047), X.int_uniform(torch.Generator().manual_seed(8), (Co,), 2047)
    for acc in (0, 1):
        dx = nan_out((B, H, W, Cc), BF16)
        dw = base_w.to(DEV) if acc else nan_out((Co, Cc))
        db = base_b.to(DEV) if acc else nan_out((Co,))
        L.check(lib.sd_head_bwd_bf16(dyd.data_ptr(), x16.data_ptr(), wd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), B, H * W, Cc, Co, acc,
                                     ws.data_ptr(), ws.numel(), L.stream()))
        same(dx, p["dx"], True, f"head bf16 dx {case}")
        X.assert_equal_report(dw, (p["dw"] + (base_w.double() if acc else 0)).float(), f"head bf16 dw {case} accumulate={acc}", "co, c")
        X.assert_equal_report(db, (p["db"] + (base_b.double() if acc else 0)).float(), f"head bf16 dbias {case} accumulate={acc}", "co")


@pytest.mark.parametrize("case", X.EXACT_FUSED_HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_fused_into_the_fpn_conv(case):
    """sd_head_split_bf16 + sd_conv2d_fwd_bf16_head (k_conv3x3_bf16_pp_head).  This kernel rounds an intermediate to bf16 on purpose: the FPN
    conv output relu(conv * scale + shift) is rounded to bf16 -- the tensor the unfused path stores -- before the head multiplies it
    (csrc/sd_conv.hip, the HEAD comment above pp_epilogue_bf16: "the rounded bf16 rows of a pass are written back ... and multiplied by the
    head weights").  The reference applies the same nearest-even rounding at the same place; the head sum on top of it is exact."""
    B, H, W, cin, co = case
    geom = (B, H, W, cin, 128, 3, 1, 1)
    L, lib, d = lib_and_desc(geom)
    p = X.fwd_problem(geom, "round")
    X.assert_exact_reference(p["ref"], p["bound"], what=str(geom))
    scale, shift, _ = X.epilogue_operands(geom, 128, (1,))
    fpn = X.epilogue_ref(p["ref"], scale, shift, None, True)
    X.assert_exact_reference(fpn, X.epilogue_bound(p["bound"], scale, shift), X.EXACT_LIMIT_HALVES, "fpn conv")
    fpn16 = X.bf16_rne(fpn.float()).double()
    g = torch.Generator().manual_seed(co)
    hw, hb = X.int_uniform(g, (co, 128), 15), X.int_uniform(g, (co,), 63)
    want = torch.einsum("bchw,oc->bohw", fpn16, hw.double()) + hb.double().view(1, -1, 1, 1)
    bound = torch.einsum("bchw,oc->bohw", fpn16.abs(), hw.double().abs()) + hb.double().abs().view(1, -1, 1, 1)
    X.assert_exact_reference(want, bound, X.EXACT_LIMIT_HALVES, "fused head")
    with X.dispatch_options(lib, {"conv_pp_min_tiles": 1, "conv_fwd_split_k": 0}):
        assert kname(lib, d, 16) == "k_conv3x3_bf16_pp"
        assert lib.sd_conv2d_fwd_bf16_head_supported(C.byref(d), co) == 1
        xd, wd, sc, sh, hwd, hbd = to_nhwc(p["x"], BF16), to_nhwc(p["w"], BF16), scale.to(DEV), shift.to(DEV), hw.to(DEV), hb.to(DEV)
        prep = torch.empty(lib.sd_head_split_bf16_bytes(), dtype=torch.uint8, device=DEV)
        L.check(lib.sd_head_split_bf16(hwd.data_ptr(), hbd.data_ptr(), co, prep.data_ptr(), L.stream()))
        out = nan_out((B, co, H, W))
        L.check(lib.sd_conv2d_fwd_bf16_head(xd.data_ptr(), wd.data_ptr(), C.byref(d), sc.data_ptr(), sh.data_ptr(), 1, prep.data_ptr(), co, out.data_ptr(), L.stream()))
        X.assert_equal_report(out, want.float(), f"fused head {case}", "b, co, y, x")
        # the unfused pair on the same operands gives the same bits
        y = nan_out((B, H, W, 128), BF16)
        L.check(lib.sd_conv2d_fwd_bf16(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), C.byref(d), sc.data_ptr(), sh.data_ptr(), 0, 0, 1, 0, 0, L.stream()))
        out2 = nan_out((B, co, H, W))
        L.check(lib.sd_head_fwd_bf16(y.data_ptr(), hwd.data_ptr(), hbd.data_ptr(), out2.data_ptr(), B, H * W, 128, co, L.stream()))
        X.assert_equal_report(out2, want.float(), f"unfused head {case}", "b, co, y, x")
