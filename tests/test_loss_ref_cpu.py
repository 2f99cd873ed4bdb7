"""CPU checks of tests/loss_ref.py: the fp64 loss reference against the fp32 oracle, the committed goldens and a torch-autograd evaluation
in double; the measured deviations behind BOUNDS; the preconditions of the exact regime; that every shape and hand-made case reaches the
branch its id names."""
import numpy as np
import pytest
import torch

from oracle import sdnet_oracle as O
from tests import loss_ref as R
from tests.helpers import ENC_KEYS

FNS = ("mse", "focal")


def _autograd_double(head, tg, M, N, fn, weights, go):
    """Loss.forward written with torch ops in double, differentiated by autograd (indices pre-clamped: gather would raise)."""
    x = head.double().requires_grad_(True)
    B, C4, h, w = x.shape
    hw, C = h * w, M + N
    hm_w, off_w, emb_w = (R.f32(v) for v in weights)
    s = torch.clamp(torch.sigmoid(x[:, :C]), min=R.CLAMP_LO, max=R.CLAMP_HI)

    def hm(p, t):
        if fn == "mse":
            return torch.nn.functional.mse_loss(p, t)
        pos, neg = (t == 1).double(), (t < 1).double()
        neg_loss = (torch.log(1 - p) * p ** 2 * (1 - t) ** 4 * neg).sum()
        if pos.sum() == 0:
            return -neg_loss
        return -((torch.log(p) * (1 - p) ** 2 * pos).sum() + neg_loss) / pos.sum()

    def l1(feat, t, inds, mask):
        if mask.sum() == 0:
            return feat.sum() * 0
        g = feat.reshape(B, 2, hw).gather(2, inds.clamp(0, hw - 1)[:, None, :].expand(-1, 2, -1)).permute(0, 2, 1)
        return ((g - t.double()).abs() * mask[..., None]).sum() / mask.sum()

    v_hm = hm_w * (hm(s[:, :M], tg["anchor_hm"].double()) + hm(s[:, M:], tg["part_hm"].double()))
    v_off = off_w * (l1(x[:, C:C + 2], tg["anchor_offsets"], tg["anchor_inds"], tg["anchor_mask"])
                     + l1(x[:, C:C + 2], tg["part_offsets"], tg["part_inds"], tg["part_mask"]))
    v_emb = emb_w * l1(x[:, C + 2:], tg["embeddings"], tg["part_inds"], tg["part_mask"])
    total = v_hm + v_off + v_emb
    (total * R.f32(go)).backward()
    return [float(v.detach()) for v in (total, v_hm, v_off, v_emb)], x.grad


@pytest.mark.parametrize("fn", FNS)
def test_oracle_deviation_sets_the_bounds(fn):
    """The fp32 oracle (torch CPU, autograd) against the fp64 reference over the whole case table, per quantity class: the largest
    deviation is what BOUNDS[fn] is 16 x of, so the oracle alone stays within bound / 16.  The reference marks as cut off by the clamp
    exactly the cells the generator planted."""
    worst = {}
    for name in R.case_table():
        c = R.table_case(name)
        ref = R.table_reference(name, fn)
        assert torch.equal(ref.sat, c.planted), name
        assert c.planted.flatten(2).double().mean(2).max().item() <= R.SAT_SHARE_CAP
        o = O.loss(c.head, c.targets, c.M, c.N, hm_loss_fn=fn, want_grad=True)
        d = R.deviations(ref, [o["total"], o["hm"], o["offset"], o["embedding"]], torch.from_numpy(o["grad"]), c.targets, c.M, c.N)
        assert (o["grad"][:, :c.M + c.N][c.planted.numpy()] == 0).all(), name
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= max(R.BOUNDS[fn][k], R.FLOOR) / 16, f"{name} {fn} {k}: oracle deviation {v:.3e} above bound / 16"
    print(f"oracle deviation {fn} " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert set(worst) == set(R.BOUNDS[fn]) and all(R.BOUNDS[fn][k] >= R.FLOOR for k in worst)


def test_case_table_covers_what_it_claims():
    t = R.case_table()
    assert len(t) == 37 and {(c["h"], c["w"]) for c in t.values()} == set(R.SHAPES.values())
    for shape in R.SHAPES.values():
        mine = [c for c in t.values() if (c["h"], c["w"]) == shape]
        assert {c["B"] for c in mine} >= {1, 3} and {(c["M"], c["N"]) for c in mine} == {(1, 1), (2, 1), (3, 5)}
    assert {c["peaks"] for c in t.values()} == set(R.PEAKS) and any(c["all_masked"] for c in t.values())
    big = t["finalize_stride_320_partials-b20-m3n5"]
    assert big["B"] * (big["M"] + big["N"]) * R.chunk_plan(big["h"] * big["w"]).chunks > 256
    for name, kw in t.items():
        c = R.table_case(name)
        hm = torch.cat([c.targets["anchor_hm"], c.targets["part_hm"]], 1)
        for has, sl in ((kw["peaks"] in ("both", "anchor"), slice(0, c.M)), (kw["peaks"] in ("both", "part"), slice(c.M, None))):
            assert bool((hm[:, sl] == 1).any()) == has
            assert not has or (hm[:, sl] == R.BELOW_ONE).any()
        assert float(hm.min()) >= 0 and float(hm.max()) <= 1 and float(c.head[:, :c.M + c.N][~c.planted].abs().max()) <= 4
    seen = {float(v) for n in t for v in R.table_case(n).head[:, :R.table_case(n).M + R.table_case(n).N][R.table_case(n).planted].tolist()}
    assert seen == set(R.SATURATED) and not any(13 < abs(v) < 14.5 for v in seen)


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_each_shape_reaches_the_chunk_case_its_id_names(name):
    h, w = R.SHAPES[name]
    p = R.chunk_plan(h * w)
    want = {"one_float4": lambda: p.chunks == 1 and p.last == 4 and p.live_last_pass == 1,
            "idle_threads_384": lambda: p.chunks == 1 and p.passes == 1 and p.live_last_pass == 96,
            "exactly_one_pass_1024": lambda: p.chunks == 1 and p.last == 1024 and p.passes == 1 and p.live_last_pass == 256,
            "two_chunks_tail_of_4": lambda: p.chunks == 2 and p.last == 4,
            "whole_chunks_8192": lambda: p.chunks == 2 and p.last == 4096 and p.passes == 4,
            "tail_chunk_of_4092": lambda: p.chunks == 2 and p.last == 4092 and p.passes == 4 and p.live_last_pass == 255}[name]
    assert want() and (h * w) % 4 == 0 and h * w <= 8192, vars(p)
    assert R.workspace_bytes(3, 3, 5, h, w) == -(-3 * 8 * p.chunks * 12 // 256) * 256


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("tag", ["scene_cfg512", "scene_small256"])
def test_reference_equals_the_goldens(golden_dir, tag, fn):
    """The recorded results of the reference implementation, at the project's 1e-4 (tests/test_gpu_parity.py::test_loss_vs_golden)."""
    g = np.load(golden_dir / f"{tag}.npz")
    W, H, M, N, K, P = (int(v) for v in g["cfg"])
    tg = {k: torch.from_numpy(np.stack([g[f"enc{n}_{k}"] for n in range(g["head"].shape[0])])) for k in ENC_KEYS}
    ref = R.loss_reference(torch.from_numpy(g["head"]), tg, M, N, fn)
    np.testing.assert_allclose(ref.out8[:4], g[f"loss_{fn}"], rtol=1e-4, atol=1e-7)
    gref = g[f"lossgrad_{fn}"]
    np.testing.assert_allclose(ref.dhead.numpy(), gref, rtol=1e-4, atol=1e-4 * np.abs(gref).max())
    assert ref.out8[6] == int(tg["anchor_mask"].sum()) and ref.out8[7] == int(tg["part_mask"].sum())
    if fn == "focal":
        assert ref.out8[4] == int((tg["anchor_hm"] == 1).sum()) and ref.out8[5] == int((tg["part_hm"] == 1).sum())


@pytest.mark.parametrize("go", [1.0, 0.37])
@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("name", ["one_float4-b3-m2n1", "idle_threads_384-b1-m3n5", "idle_threads_384-b3-m1n1", "exactly_one_pass_1024-b1-m1n1",
                                  "exactly_one_pass_1024-b1-m2n1", "two_chunks_tail_of_4-b3-m3n5"])
def test_reference_equals_torch_autograd_in_double(name, fn, go):
    """To 1e-12, values and every gradient group (saturated cells included: both give exactly 0 there)."""
    c = R.table_case(name)
    ref = R.loss_reference(c.head, c.targets, c.M, c.N, fn, c.weights, go)
    vals, grad = _autograd_double(c.head, c.targets, c.M, c.N, fn, c.weights, go)
    for i in range(4):
        assert abs(vals[i] - ref.out8[i]) <= 1e-12 * abs(vals[i])
    C = c.M + c.N
    for sl in (slice(0, c.M), slice(c.M, C), slice(C, C + 2), slice(C + 2, C + 4)):
        assert float((grad[:, sl] - ref.dhead[:, sl]).abs().max()) <= 1e-12 * float(grad[:, sl].abs().max())
    assert (ref.dhead[:, :C][ref.sat] == 0).all() and (grad[:, :C][ref.sat] == 0).all()


def test_peak_configurations_of_the_autograd_check():
    names = ["one_float4-b3-m2n1", "idle_threads_384-b1-m3n5", "idle_threads_384-b3-m1n1", "exactly_one_pass_1024-b1-m1n1",
             "exactly_one_pass_1024-b1-m2n1", "two_chunks_tail_of_4-b3-m3n5"]
    assert {R.case_table()[n]["peaks"] for n in names} == set(R.PEAKS)


def test_reference_states_the_index_clamp():
    """Indices below 0 and above hw - 1 give what indices 0 and hw - 1 give (the oracle's gather would raise on them)."""
    c = R.SCATTER_CASES["index_clamp_minus5_hw_plus7"]()
    hw = c.h * c.w
    assert int(c.targets["anchor_inds"].min()) == -5 and int(c.targets["anchor_inds"].max()) == hw + 7
    clamped = dict(c.targets, anchor_inds=c.targets["anchor_inds"].clamp(0, hw - 1), part_inds=c.targets["part_inds"].clamp(0, hw - 1))
    a, b = R.loss_reference(c.head, c.targets, c.M, c.N, "mse", c.weights), R.loss_reference(c.head, clamped, c.M, c.N, "mse", c.weights)
    assert np.array_equal(a.out8, b.out8) and torch.equal(a.dhead, b.dhead) and a.out8[2] > 0
    o = O.loss(c.head, clamped, c.M, c.N, hm_weight=c.weights[0], offset_weight=c.weights[1], embedding_weight=c.weights[2], want_grad=True)
    assert np.array_equal(np.float32(a.out8[:4]), np.float32([o["total"], o["hm"], o["offset"], o["embedding"]]))


def test_sigmoid_never_equals_the_upper_clamp_bound():
    """1 + expf(-x) is 1 + k 2^-23 in fp32 and 1 / (1 + k 2^-23) rounds to 1 - 16 u (k = 8) or 1 - 18 u (k = 9), never to the bound
    1 - 17 u: whether the clamp's backward includes its upper bound cannot be observed through this sigmoid, and the lower bound is met
    only at logits inside the band the random regime leaves out."""
    f = np.float32
    assert f(R.CLAMP_HI) == f(1) - f(17 * R.U)
    got = {float(f(1) / (f(1) + f(k * 2.0 ** -23))) for k in range(0, 64)}
    assert R.CLAMP_HI not in got and float(f(1) - f(16 * R.U)) in got and float(f(1) - f(18 * R.U)) in got


# ---- the exact regime -------------------------------------------------------------------------------------------------------------
EXACT = [(B, M, N, h, w) for (h, w) in R.SHAPES.values() for (B, M, N) in ((1, 1, 1), (3, 3, 5))] + [(20, 3, 5, 89, 92)]


@pytest.mark.parametrize("B,M,N,h,w", EXACT)
def test_exact_inputs_keep_every_sum_exact(B, M, N, h, w):
    c = R.exact_case(B, M, N, h, w, seed=h)
    hw, C = h * w, M + N
    assert not c.head[:, :C].any()
    t = torch.cat([c.targets["anchor_hm"], c.targets["part_hm"]], 1).double()
    assert set(t.unique().tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
    term = (0.5 - t) ** 2
    assert torch.equal(term * 16, (term * 16).round())
    # any partial sum inside one chunk, in any order, is a multiple of 1/16 below 4096 / 4: exact in fp32; across chunks the kernel adds in double
    assert 0.25 * R.LOSS_CHUNK * 16 < 2 ** 24
    for k in ("anchor_offsets", "part_offsets", "embeddings"):
        assert torch.equal(c.targets[k] * 8, (c.targets[k] * 8).round()) and float(c.targets[k].abs().max()) <= 8
    reg = c.head[:, C:]
    assert torch.equal(reg * 8, (reg * 8).round())
    for wgt in c.weights:
        assert np.log2(wgt) == round(np.log2(wgt))
    ref = R.loss_reference(c.head, c.targets, M, N, "mse", c.weights)
    want = R.exact_out8(c)
    assert np.array_equal(ref.out8.astype(np.float32), want) and want[2] > 0 and want[3] > 0 and want[6] >= 3 and want[7] >= 4
    # duplicates within and across the lists, and entries with dx == 0
    ai, pi = c.targets["anchor_inds"], c.targets["part_inds"]
    assert torch.equal(ai[:, 0], ai[:, 1]) and torch.equal(ai[:, 0], pi[:, 0])
    bi = torch.arange(B)
    assert torch.equal(c.targets["anchor_offsets"][:, 2], c.head.view(B, C + 4, hw)[bi, C:C + 2, ai[:, 2]])
    for go in (1.0, 2.0 ** -3, 2.0 ** 10):
        d = torch.from_numpy(R.exact_dhead(c, go)).double()
        r = R.loss_reference(c.head, c.targets, M, N, "mse", c.weights, go).dhead
        assert float(((d - r).abs() - 8 * R.U * r.abs()).max()) <= 0          # one rounded division, up to a handful of duplicates
        assert torch.equal(d == 0, r == 0)
        assert torch.equal(d, torch.from_numpy(R.exact_dhead(c, 1.0)).double() * go) and float(d[d != 0].abs().min()) > 2.0 ** -100


@pytest.mark.parametrize("h,w", [(41, 100), (89, 92)])
def test_onehot_sweep_rows(h, w):
    M, N = 3, 5
    case, where, rows = R.onehot_sweep(M, N, h, w)
    hw = h * w
    assert {p for _, p in where} >= {0, 3, 4, 1020, 1023, 1024, 4092, 4095, 4096, hw - 4, hw - 1} and {c for c, _ in where} == {0, 2, 3, 7}
    for b, (c, p) in enumerate(where):
        want = np.float32(0.25 / ((M if c < M else N) * hw))
        assert rows[b, 0] == want and rows[b, 1] == want and not rows[b, 2:].any()
    for b in range(0, case.B, 7):
        one = {k: v[b:b + 1] for k, v in case.targets.items()}
        ref = R.loss_reference(case.head[b:b + 1], one, M, N, "mse", case.weights)
        assert np.array_equal(ref.out8.astype(np.float32), rows[b])


@pytest.mark.parametrize("name", list(R.SCATTER_CASES))
def test_scatter_cases_hold_what_their_ids_name(name):
    c = R.SCATTER_CASES[name]()
    hw, C = c.h * c.w, c.M + c.N
    tg = c.targets
    ca, cp = int(tg["anchor_mask"].sum()), int(tg["part_mask"].sum())
    wa, wp, we = R.scatter_weights_f32(1.0, c.weights[1], c.weights[2], ca, cp)
    exp = R.scatter_expected(c, 1.0)
    ref = R.loss_reference(c.head, tg, c.M, c.N, "mse", c.weights)
    r = ref.dhead[:, C:].reshape(c.B, 4, hw)
    assert float(((torch.from_numpy(exp).double() - r).abs() - 8 * R.U * r.abs()).max()) <= 0
    assert np.array_equal(ref.out8.astype(np.float32), R.exact_out8(c))
    values = set(np.abs(exp[exp != 0]).tolist())
    if name == "single_entry_signs":
        assert exp[0, 0, 5] == wa and exp[0, 1, 5] == -wa and not exp[0, :, 9].any() and exp[0, 0, 13] == -wa and exp[0, 1, 13] == 0
        assert exp[0, 0, 20] == -wp and exp[0, 2, 20] == 0 and exp[0, 3, 20] == -we and values == {float(wa), float(wp), float(we)}
    elif name == "two_anchors_one_cell":
        assert exp[0, 0, 7] == wa + wa and exp[0, 1, 7] == 0 and ca == 3
    elif name == "anchor_part_cancel_to_zero":
        assert ca == cp and wa == wp and wa > 0 and not exp[0, :2, 11].any() and exp[0, 2, 11] == -we
    elif name == "anchor_part_different_weights":
        assert ca != cp and exp[0, 0, 11] == np.float32(wa + wp) and exp[0, 1, 11] == np.float32(-wa + wp)
    elif name == "three_duplicates_list_order":
        assert (ca, cp) == (3, 7) and (exp != R.scatter_expected(c, 1.0, reverse=True)).any()
    elif name == "masked_off_duplicate_ignored":
        assert exp[0, 0, 70] == wa and exp[0, 0, 72] == wp and (ca, cp) == (2, 1)
    elif name == "index_clamp_minus5_hw_plus7":
        assert exp[0, 0, 0] == np.float32(wa + wp) and exp[0, 0, hw - 1] == np.float32(-wa - wp) and exp[0, 1, 0] == np.float32(wa - wp)
    elif name == "all_masks_off":
        assert not exp.any() and ca == cp == 0 and not ref.out8[2:4].any()
    elif name == "k200_p120_duplicates_across_256":
        assert (c.K, c.P) == (200, 120) and int(tg["part_inds"][0, 100]) == int(tg["anchor_inds"][0, 10]) and 10 < 256 <= 200 + 100
        assert int(tg["part_inds"][0, 70]) == int(tg["part_inds"][0, 50]) and 200 + 50 < 256 <= 200 + 70
    elif name == "p300_embedding_stride":
        assert c.P == 300 and int(tg["part_inds"][0, 299]) == int(tg["part_inds"][0, 3]) and int(tg["part_inds"][0, 280]) == int(tg["part_inds"][0, 260])
    elif name == "l1_term_b3_k100_stride":
        assert c.B * c.K > 256 and ca == 300


def test_render_reference_equals_the_oracle_merge():
    """min d^2 first, one exp: the same values as the oracle's full-frame Gaussians merged with an elementwise max."""
    h, w, sigma = 12, 20, 1.7
    cx, cy = [3, 15, -3, 22, 7], [2, 9, 5, -2, 11]
    d2 = R.min_d2(cx, cy, h, w)
    ref = R.render_reference(d2, np.float32(2 * sigma ** 2))
    merged = np.max([O.gaussian_2d(h, w, x, y, sigma) for x, y in zip(cx, cy)], 0)
    np.testing.assert_allclose(merged, ref, rtol=2e-7, atol=0)
    assert ref[2, 3] == 1.0 and ref[9, 15] == 1.0 and R.min_d2([], [], h, w) is None
