"""sd_loss_fwd / sd_loss_fwd_per_image / sd_loss_bwd and sd_render_targets through the C ABI against tests/loss_ref.py, branch by branch.

Exact regime (logits 0, targets from {0, 1/4, 1/2, 3/4, 1}, dyadic regression values, power-of-two weights): every output equals the
restated value bit for bit -- a dropped or doubled float4 at a chunk tail, a wrong count in a weight, an omitted or reordered duplicate
sum all change a bit.  Random regime: values and the gradient of each channel group within loss_ref.BOUNDS (16 x the measured deviation
of the fp32 CPU oracle) of the fp64 reference; saturated logits give exactly 0.  out8[4..7] are compared with the integer counts in
every test.  dhead, out8 and the workspace (exactly sd_loss_workspace_bytes) start as NaN and are followed by a guard region of a
sentinel inside the same allocation; after every call the guards and all inputs are unchanged and no NaN is left in dhead.

Each toleranced check prints `loss err/bound <case> <quantity> <ratio>`; docs/DESIGN_LOG.md holds the table of one run."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests.helpers import assert_equal_report

pytestmark = pytest.mark.gpu
DEV = "cuda"
FN = {"mse": 0, "focal": 1}
SD_ERR_INVALID, SD_ERR_WORKSPACE, SD_ERR_ALIGN = -1, -2, -3          # include/sdnet_hip.h
GUARD, SENTINEL, WS_GUARD_BYTE = 256, 12345.0, 0xA5
LAYOUTS = ("contiguous", "head_channel_slice", "targets_padded_batch", "targets_every_other_channel")
HM_KEYS = (("anchor_hm", "t_anchor_hm", "ta"), ("part_hm", "t_part_hm", "tp"))
_KEEP = []   # device tensors whose raw pointers go to the C ABI outlive the launch: released after the test's last synchronisation


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def keep(t):
    _KEEP.append(t)
    return t


def guarded(n):
    """n NaN floats followed by GUARD sentinel floats in one allocation."""
    buf = keep(torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV))
    buf[:n] = float("nan")
    return buf


def fresh(t):
    """A new device tensor with the standard contiguous strides (a clone of a one-image or one-channel slice would keep its parent's)."""
    return torch.empty(t.shape, dtype=t.dtype, device=DEV).copy_(t)


def guard_intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def report(case, what, err, bound):
    print(f"loss err/bound {case} {what} {err / bound:.4g}")


class Placed:
    """One case on the device in one stride layout, its descriptor built by the package's own loss_desc (so only views that
    _lib.map_view passes through without a copy reach the kernels -- asserted), and the three entry points with guarded outputs."""

    def __init__(self, case, fn, layout="contiguous"):
        from structuredetector_amd import _lib as L
        from structuredetector_amd.model.loss import loss_desc
        self.L, self.lib, self.case = L, L.lib(), case
        B, M, N, h, w = case.B, case.M, case.N, case.h, case.w
        hw, C4 = h * w, M + N + 4
        self.shape = (B, C4, h, w)
        if layout == "head_channel_slice":            # the head as channels 2 .. 2 + C4 of a wider buffer: sb > C4 * hw
            head_buf = torch.full((B, C4 + 5, h, w), 3.25, device=DEV)
            head = head_buf[:, 2:2 + C4]
            head.copy_(case.head)
        else:
            head_buf = head = fresh(case.head)
        tg = {k: fresh(v) for k, v in case.targets.items()}
        self.bufs = [head_buf]
        for k, Cg in (("anchor_hm", M), ("part_hm", N)):
            if layout == "targets_padded_batch":      # one more channel per image than the kernels are told about
                buf = torch.full((B, Cg + 1, h, w), 1.0, device=DEV)
                view = buf[:, :Cg]
            elif layout == "targets_every_other_channel":
                buf = torch.full((B, 2 * Cg, h, w), 1.0, device=DEV)
                view = buf[:, ::2]
            else:
                buf = view = tg[k]
            if buf is not view:
                view.copy_(tg[k])
                tg[k] = view
            self.bufs.append(buf)
        self.bufs += [tg[k] for k in tg if not k.endswith("_hm")]
        self.desc, self.keep = loss_desc(head, tg, (M, N, case.K, case.P, FN[fn], *case.weights))
        d = self.desc
        assert (d.anchor_hm, d.a_sb, d.a_sc) == (head.data_ptr(), head.stride(0), hw) and d.offsets == head.data_ptr() + 4 * (M + N) * hw
        for k, field, pre in HM_KEYS:
            assert getattr(d, field) == tg[k].data_ptr(), f"{layout}: map_view copied {k}"
            assert (getattr(d, pre + "_sb"), getattr(d, pre + "_sc")) == (tg[k].stride(0), tg[k].stride(1))
        Cs = {"ta": M, "tp": N}
        want = {"contiguous": lambda p: (Cs[p] * hw, hw), "head_channel_slice": lambda p: (Cs[p] * hw, hw),
                "targets_padded_batch": lambda p: ((Cs[p] + 1) * hw, hw), "targets_every_other_channel": lambda p: (2 * Cs[p] * hw, 2 * hw)}[layout]
        assert all((getattr(d, p + "_sb"), getattr(d, p + "_sc")) == want(p) for p in ("ta", "tp"))
        assert d.a_sb == ((C4 + 5) * hw if layout == "head_channel_slice" else C4 * hw)
        for k in ("anchor_inds", "part_inds", "anchor_offsets", "part_offsets", "anchor_mask", "part_mask"):
            assert getattr(d, k) == tg[k].data_ptr()
        assert d.t_embeddings == tg["embeddings"].data_ptr()
        self.snapshot = [b.clone() for b in self.bufs]
        keep(self)

    def inputs_unchanged(self):
        return all(torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a, b.view(torch.uint8) if b.dtype == torch.bool else b)
                   for a, b in zip(self.bufs, self.snapshot))

    def workspace(self):
        d = self.desc
        nbytes = self.lib.sd_loss_workspace_bytes(d.B, d.M, d.N, d.h, d.w)
        assert nbytes == R.workspace_bytes(d.B, d.M, d.N, d.h, d.w)
        ws = keep(torch.full((nbytes + GUARD,), WS_GUARD_BYTE, dtype=torch.uint8, device=DEV))
        ws[:nbytes] = 0xFF                                                      # all-ones words: NaN
        return ws, nbytes

    def forward(self, per_image=False):
        """-> (rows, 8) float32 on the device (rows = 1 for sd_loss_fwd)."""
        rows = self.desc.B if per_image else 1
        ws, nbytes = self.workspace()
        out = guarded(rows * 8)
        f = self.lib.sd_loss_fwd_per_image if per_image else self.lib.sd_loss_fwd
        self.L.check(f(C.byref(self.desc), out.data_ptr(), ws.data_ptr(), nbytes, self.L.stream()), "sd_loss_fwd")
        torch.cuda.synchronize()
        assert guard_intact(out, rows * 8), "the forward wrote past its outputs"
        assert bool((ws[nbytes:] == WS_GUARD_BYTE).all()), "the forward wrote past sd_loss_workspace_bytes"
        assert self.inputs_unchanged(), "the forward changed an input"
        return out[:rows * 8].view(rows, 8)

    def backward(self, out8, go):
        n = int(np.prod(self.shape))
        dh = guarded(n)
        g = keep(torch.tensor([go], dtype=torch.float32, device=DEV))
        self.L.check(self.lib.sd_loss_bwd(C.byref(self.desc), out8.data_ptr(), g.data_ptr(), dh.data_ptr(), self.L.stream()), "sd_loss_bwd")
        torch.cuda.synchronize()
        assert not torch.isnan(dh[:n]).any(), f"sd_loss_bwd left {int(torch.isnan(dh[:n]).sum())} elements of dhead unwritten"
        assert guard_intact(dh, n), "sd_loss_bwd wrote past dhead"
        assert self.inputs_unchanged(), "sd_loss_bwd changed an input"
        return dh[:n].view(self.shape)


def one_image(case, b):
    from types import SimpleNamespace
    return SimpleNamespace(**{**vars(case), "B": 1, "head": case.head[b:b + 1], "targets": {k: v[b:b + 1] for k, v in case.targets.items()}})


def assert_rows_equal_single_image_calls(case, fn, rows, images=None):
    """Row b of sd_loss_fwd_per_image has the bits of sd_loss_fwd on image b alone."""
    for b in (range(case.B) if images is None else images):
        single = Placed(one_image(case, b), fn).forward()
        assert torch.equal(single[0], rows[b]), f"per-image row {b}: {rows[b].tolist()} != B = 1 forward {single[0].tolist()}"


def bits_equal(got, want, what):
    assert_equal_report(got, torch.from_numpy(np.ascontiguousarray(want)), what, layout="bchw")


# ---- exact regime ------------------------------------------------------------------------------------------------------------------
EXACT = [(B, M, N, h, w) for (h, w) in R.SHAPES.values() for (B, M, N) in ((1, 1, 1), (3, 3, 5))] + [(20, 3, 5, 89, 92)]


def run_exact(case, tag, layout="contiguous"):
    """mse on an exact-regime case: out8 (counts included), the per-image rows and the whole of dhead, bit for bit."""
    p = Placed(case, "mse", layout)
    out8 = p.forward()
    want = R.exact_out8(case)
    assert np.array_equal(out8[0].cpu().numpy(), want), f"{tag}: out8 {out8[0].tolist()} != {want.tolist()}"
    assert want[4] == 0 and want[5] == 0 and want[6] == int(case.targets["anchor_mask"].sum()) and want[7] == int(case.targets["part_mask"].sum())
    rows = p.forward(per_image=True)
    for b in range(case.B):
        assert np.array_equal(rows[b].cpu().numpy(), R.exact_out8(one_image(case, b))), f"{tag}: per-image row {b}"
    assert_rows_equal_single_image_calls(case, "mse", rows)
    d1 = p.backward(out8, 1.0)
    bits_equal(d1, R.exact_dhead(case, 1.0), f"{tag} dhead")
    for go in (2.0 ** -3, 2.0 ** 10):
        dg = p.backward(out8, go)
        assert torch.equal(dg, d1 * go), f"{tag}: dhead({go}) != {go} * dhead(1)"
        bits_equal(dg, R.exact_dhead(case, go), f"{tag} dhead grad_out={go}")
    return d1


@pytest.mark.parametrize("i", range(len(EXACT)), ids=[f"b{B}-m{M}n{N}-{h}x{w}" for B, M, N, h, w in EXACT])
def test_exact_mse_forward_and_backward(i):
    """Every SHAPES plane (one float4, idle threads, one full pass, two chunks with a 4-element and a 4092-element tail, whole chunks) at
    B = 1, (1, 1) and B = 3, (3, 5), the 320-partial finalize, the four stride layouts cycled through them: hm = fp32(hm_w (Sa / (B M hw) +
    Sp / (B N hw))) from the integer sums, the dyadic L1 terms, out8[4..7], and dhead = scale (0.5 - t) / 4 with list-order scatter sums."""
    B, M, N, h, w = EXACT[i]
    run_exact(R.exact_case(B, M, N, h, w, seed=h), f"exact-b{B}-m{M}n{N}-{h}x{w}", LAYOUTS[i % len(LAYOUTS)])


@pytest.mark.parametrize("h,w", [(41, 100), (89, 92)])
def test_onehot_sweep_finds_every_float4_of_a_plane(h, w):
    """One launch, one image per (channel, position): a single term of 1/4 at positions 0, 3, 4, 1020, 1023, 1024, 4092, 4095, 4096, hw - 4,
    hw - 1 of the first and last channel of each group must arrive in that image's row as fp32(0.25 / (Cg hw)), exactly once."""
    case, where, want = R.onehot_sweep(3, 5, h, w)
    rows = Placed(case, "mse").forward(per_image=True).cpu().numpy()
    for b, (c, pos) in enumerate(where):
        assert np.array_equal(rows[b], want[b]), f"hw={h * w} channel {c} position {pos}: row {rows[b].tolist()} != {want[b].tolist()}"
    assert_rows_equal_single_image_calls(case, "mse", torch.from_numpy(rows).to(DEV), images=range(0, case.B, 5))


@pytest.mark.parametrize("name", list(R.SCATTER_CASES))
def test_scatter_cases(name):
    """k_loss_bwd_scatter and l1_term on hand-made lists at hw = 384: signs +, -, 0; duplicates within a list, across the two lists with equal
    weights (exactly 0) and different ones, three and more in list order; a masked-off entry in an occupied cell; indices -5 and hw + 7;
    all masks off; duplicates on both sides of the loops' stride of 256 (K + P = 320, P = 300); B K = 300 entries for l1_term.  Every cell of
    the four regression channels is compared: the written ones with the float32 list-order sums, all others with 0."""
    run_exact(R.SCATTER_CASES[name](), f"scatter-{name}")


# ---- random regime -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", list(FN))
@pytest.mark.parametrize("name", list(R.case_table()))
def test_random_regime_within_measured_bounds(name, fn):
    """Values and per-group gradients against the fp64 reference for grad_out 1 and 0.37 in every stride layout; counts equal; the planted
    saturated cells exactly 0 and everything finite; the layouts agree bit for bit; power-of-two grad_out scales dhead bit for bit."""
    c = R.table_case(name)
    ref = R.table_reference(name, fn)
    C = c.M + c.N
    bounds = R.BOUNDS[fn]
    counts = ref.out8[4:].astype(np.float32)
    refs = {1.0: ref, 0.37: R.loss_reference(c.head, c.targets, c.M, c.N, fn, c.weights, 0.37)}
    first = None
    for layout in LAYOUTS:
        tag = f"{name}-{fn}-{layout}"
        p = Placed(c, fn, layout)
        out8 = p.forward()
        o = out8[0].cpu().numpy()
        assert np.isfinite(o).all() and np.array_equal(o[4:], counts), f"{tag}: counts {o[4:].tolist()} != {counts.tolist()}"
        grads = {go: p.backward(out8, go) for go in (1.0, 0.37)}
        for go, dh in grads.items():
            dh = dh.cpu()
            assert torch.isfinite(dh).all() and not dh[:, :C][c.planted].any(), f"{tag}: gradient through a saturated sigmoid"
            dev = R.deviations(refs[go], o[:4], dh, c.targets, c.M, c.N)
            for k, v in dev.items():
                if k == "value" and go != 1.0:
                    continue
                report(tag, f"{k}{'' if go == 1.0 else '_go0.37'}", v, bounds[k])
                assert v <= bounds[k], f"{tag} grad_out={go} {k}: deviation {v:.3e} above the bound {bounds[k]:.3e} ({v / bounds[k]:.3g} x)"
        if first is None:
            first = (out8.clone(), {go: g.clone() for go, g in grads.items()})
            rows = p.forward(per_image=True)
            for b in range(c.B):
                rb = R.loss_reference(c.head[b:b + 1], {k: v[b:b + 1] for k, v in c.targets.items()}, c.M, c.N, fn, c.weights).out8
                assert np.array_equal(rows[b, 4:].cpu().numpy(), rb[4:].astype(np.float32)), f"{tag}: per-image counts of image {b}"
            assert_rows_equal_single_image_calls(c, fn, rows, images=range(min(c.B, 3)))
            for go in (2.0 ** -3, 2.0 ** 10):
                assert torch.equal(p.backward(out8, go), grads[1.0] * go), f"{tag}: dhead({go}) != {go} * dhead(1)"
            assert float(grads[1.0][grads[1.0] != 0].abs().min()) > 2.0 ** -123      # 2^-3 times that is still a normal number
        else:
            assert torch.equal(out8, first[0]) and all(torch.equal(grads[go], first[1][go]) for go in grads), f"{tag}: differs from the contiguous layout"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusal_codes_and_nothing_written():
    """One case per refusal code of check_desc / the entry points: h * w no multiple of 4 and an unknown loss function (invalid), a workspace
    one byte short, a stride that is no multiple of 4 and pointers off by 4 bytes (alignment).  A refused call writes nothing."""
    c = R.exact_case(1, 2, 1, 16, 24, seed=3)
    p = Placed(c, "mse")
    lib, L = p.lib, p.L
    ws, nbytes = p.workspace()
    out, dh = guarded(8), guarded(int(np.prod(p.shape)))
    g = keep(torch.ones(1, device=DEV))
    good = keep(p.forward().clone())

    def variant(**kw):
        d = type(p.desc).from_buffer_copy(p.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    fwd = lambda d, nb=nbytes, o=out: lib.sd_loss_fwd(C.byref(d), o.data_ptr(), ws.data_ptr(), nb, L.stream())
    bwd = lambda d, dst: lib.sd_loss_bwd(C.byref(d), good.data_ptr(), g.data_ptr(), dst, L.stream())
    assert fwd(variant(h=3, w=3)) == SD_ERR_INVALID and b"multiple of 4" in lib.sd_last_error()
    assert fwd(variant(hm_loss_fn=2)) == SD_ERR_INVALID and bwd(variant(hm_loss_fn=2), dh.data_ptr()) == SD_ERR_INVALID
    assert fwd(p.desc, nbytes - 1) == SD_ERR_WORKSPACE
    assert lib.sd_loss_fwd_per_image(C.byref(p.desc), out.data_ptr(), ws.data_ptr(), nbytes - 1, L.stream()) == SD_ERR_WORKSPACE
    assert fwd(variant(a_sb=p.desc.a_sb + 2)) == SD_ERR_ALIGN and fwd(variant(tp_sc=p.desc.tp_sc + 1)) == SD_ERR_ALIGN
    assert fwd(variant(t_anchor_hm=p.desc.t_anchor_hm + 4)) == SD_ERR_ALIGN
    assert bwd(p.desc, dh.data_ptr() + 4) == SD_ERR_ALIGN
    torch.cuda.synchronize()
    assert torch.isnan(out[:8]).all() and torch.isnan(dh[:-GUARD]).all() and guard_intact(out, 8) and bool((ws[:nbytes] == 0xFF).all())
    assert fwd(p.desc) == 0                                   # and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert torch.equal(out[:8], good[0])


# ---- target rendering --------------------------------------------------------------------------------------------------------------
def render(scene, B, Cc, h, w, two_sigma2):
    """scene[b][c] = [(x, y), ...] -> sd_render_targets' (B, Cc, h, w) map as numpy, from a NaN-prefilled, guarded buffer."""
    from structuredetector_amd import _lib as L
    pts = [kp for b in range(B) for c in range(Cc) for kp in scene[b][c]]
    ptr = np.cumsum([0] + [len(scene[b][c]) for b in range(B) for c in range(Cc)]).astype(np.int32)
    cx = keep(torch.tensor([x for x, _ in pts] or [0], dtype=torch.int32, device=DEV))
    cy = keep(torch.tensor([y for _, y in pts] or [0], dtype=torch.int32, device=DEV))
    cp = keep(torch.from_numpy(ptr).to(DEV))
    n = B * Cc * h * w
    out = guarded(n)
    L.check(L.lib().sd_render_targets(cx.data_ptr(), cy.data_ptr(), cp.data_ptr(), B, Cc, h, w, float(np.float32(two_sigma2)), out.data_ptr(),
                                      L.stream()), "sd_render_targets")
    torch.cuda.synchronize()
    assert not torch.isnan(out[:n]).any(), "sd_render_targets left elements unwritten"
    assert guard_intact(out, n), "sd_render_targets wrote past its map"
    return out[:n].view(B, Cc, h, w).cpu().numpy()


def make_scene(h, w, many, seed):
    """B = 2, four channels: a full one (`many` keypoints inside the map), an empty one, one with centres at -3, w + 2, -3, h + 2 around
    one inside, and one that is empty in image 0 and holds a corner keypoint in image 1."""
    rng = np.random.default_rng(seed)
    inside = lambda n: [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(n)]
    scene = []
    for b in range(2):
        outside = [(-3, int(rng.integers(0, h))), (w + 2, int(rng.integers(0, h))), (int(rng.integers(0, w)), -3), (int(rng.integers(0, w)), h + 2)]
        scene.append([inside(many), [], outside + inside(1), [] if b == 0 else [(w - 1, h - 1)]])
    return scene


RENDER = {"one_quad_1x4": (1, 4, 3, 1.3), "7x36": (7, 36, 5, 2.1), "second_block_one_live_thread_1x1028": (1, 1028, 6, 3.3),
          "300_keypoints_33x124": (33, 124, 300, 3.3), "int32_limit_16384x4": (16384, 4, 4, 40.0)}


@pytest.mark.parametrize("name", list(RENDER))
def test_render_targets(name):
    """Bitwise: centres inside the map are 1.0, empty channels 0.0, equal min d^2 gives equal bits and a larger one no larger value, a
    keypoint that is nowhere nearest and a permuted keypoint order change nothing, mirrored scenes give mirrored maps.  Values against
    exp in double of the float32 quotient at the tolerance of test_encode_vs_golden."""
    h, w, many, sigma = RENDER[name]
    two_sigma2 = np.float32(2 * sigma ** 2)
    scene = make_scene(h, w, many, seed=h + w)
    B, Cc = 2, 4
    got = render(scene, B, Cc, h, w, two_sigma2)
    for b in range(B):
        for c in range(Cc):
            kps, m = scene[b][c], got[b, c]
            if not kps:
                assert not m.any() and not np.signbit(m).any(), f"{name}: empty channel ({b}, {c}) is not +0.0 everywhere"
                continue
            d2 = R.min_d2([x for x, _ in kps], [y for _, y in kps], h, w)
            np.testing.assert_allclose(m, R.render_reference(d2, two_sigma2), rtol=1e-5, atol=1e-7, err_msg=f"{name} ({b}, {c})")
            for x, y in kps:
                if 0 <= x < w and 0 <= y < h:
                    assert m[y, x] == 1.0, f"{name}: centre ({x}, {y}) of channel ({b}, {c}) is {m[y, x]!r}"
            assert ((m == 1.0) == (d2 == 0)).all()
            order = np.argsort(d2.ravel(), kind="stable")
            ds, vs = d2.ravel()[order], m.ravel()[order]
            assert (np.diff(vs) <= 0).all(), f"{name} ({b}, {c}): a value rises with min d^2"
            same = ds[1:] == ds[:-1]
            assert (vs[1:][same] == vs[:-1][same]).all(), f"{name} ({b}, {c}): equal min d^2, different values"
    far = (-(w + h + 10), -(w + h + 10))                    # farther from every pixel than any keypoint within 5 of the map
    shuffled = [[(list(reversed(kps)) + [kps[0], far]) if kps else [] for kps in img] for img in scene]
    assert np.array_equal(render(shuffled, B, Cc, h, w, two_sigma2), got), f"{name}: keypoint order or a never-nearest keypoint changes the map"
    flip_x = [[[(w - 1 - x, y) for x, y in kps] for kps in img] for img in scene]
    assert np.array_equal(render(flip_x, B, Cc, h, w, two_sigma2), got[..., ::-1]), f"{name}: x-mirrored scene"
    flip_y = [[[(x, h - 1 - y) for x, y in kps] for kps in img] for img in scene]
    assert np.array_equal(render(flip_y, B, Cc, h, w, two_sigma2), got[..., ::-1, :]), f"{name}: y-mirrored scene"
