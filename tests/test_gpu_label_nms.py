"""Cross-label anchor suppression on the GPU: `sd_label_nms` bit for bit (no tolerance: only `max` and `==` enter the definition) against
the definition restated with torch ops and the project's own primitives (tests/label_nms_ref.py), in every staging variant, on the output
of `sd_nms5` as the plain path feeds it, and the definition's consequences on planted peaks."""
import pytest
import torch

from tests.label_nms_ref import expected_label_nms, expected_nms5_labels, normal_logits, tie_logits

pytestmark = pytest.mark.gpu

# (B, M, N, h, w, R)
SHAPES = [(1, 1, 1, 8, 12, 1),
          (3, 2, 1, 7, 9, 2),
          (2, 3, 2, 16, 64, 2),            # exactly one tile
          (2, 4, 3, 40, 136, 3),           # tails on both axes, windows across tile borders
          (1, 5, 0, 33, 70, 8),            # the largest radius, w % 4 != 0, no part channel
          (1, 252, 4, 8, 8, 2),            # label-index width
          (2, 2, 1, 128, 128, 2)]          # the production map
FAMILIES = {"tie": tie_logits, "normal": normal_logits}
LAYOUTS = ("contiguous", "slice", "offset")


def lay_out(x, layout):
    """A copy of the (B, C, h, w) tensor x in one of the layouts: contiguous planes; the first C channels of a (B, C + 4, h, w) tensor; the
    same planes one float into their storage (4-byte aligned only: the 4-byte staging also where w % 4 == 0)."""
    B, C, h, w = x.shape
    if layout == "contiguous":
        t = x.clone()
    elif layout == "slice":
        t = torch.full((B, C + 4, h, w), float("nan"), device=x.device)[:, :C]
        t.copy_(x)
    else:
        t = torch.full((x.numel() + 1,), float("nan"), device=x.device)[1:].view(B, C, h, w)
        t.copy_(x)
        assert t.data_ptr() % 16 == 4
    assert torch.equal(t, x)
    return t


def run_label_nms(p, R, offset_out=False):
    from structuredetector_amd import _lib as L
    B, M, h, w = p.shape
    assert p.stride(3) == 1 and p.stride(2) == w
    buf = torch.full((p.numel() + 1,), float("nan"), device=p.device)
    out = (buf[1:] if offset_out else buf[:-1]).view(B, M, h, w)
    L.check(L.lib().sd_label_nms(p.data_ptr(), p.stride(0), p.stride(1), out.data_ptr(), B, M, h, w, R, L.stream()), "sd_label_nms")
    return out


def nms5_sigmoid(x):
    from structuredetector_amd import _lib as L
    B, C, h, w = x.shape
    out = torch.empty((B, C, h, w), device=x.device)
    L.check(L.lib().sd_nms5(x.data_ptr(), x.stride(0), x.stride(1), out.data_ptr(), B, C, h, w, 1, L.stream()), "sd_nms5")
    return out


_cache = {}


def reference(shape, family):
    """(logits, nms(clamped_sigmoid(logits)), expected_nms5_labels) of a shape and family, computed once and left unchanged."""
    key = (shape, family)
    if key not in _cache:
        B, M, N, h, w, R = shape
        x = FAMILIES[family]((B, M + N, h, w), 1000 * SHAPES.index(shape) + len(family), "cuda")
        from structuredetector_amd.utils.ops import clamped_sigmoid, nms
        _cache[key] = (x, nms(clamped_sigmoid(x)), expected_nms5_labels(x, M, R))
    return _cache[key]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_is_not_vacuous(shape, family):
    """From the reference alone: peaks are suppressed wherever there are two labels, and on the tie family the lowest-label rule decides
    cells wherever there are three."""
    B, M, N, h, w, R = shape
    x, maps, want = reference(shape, family)
    P, out = maps[:, :M], want[:, :M]
    peaks, kept = int((P > 0).sum()), int((out > 0).sum())
    best = P.max(1).values
    ties = int((((P == best[:, None]) & (best[:, None] > 0)).sum(1) > 1).sum())
    print(f"{shape} {family}: {peaks} peaks, {kept} kept, {ties} cells where labels tie")
    assert 0 < kept <= peaks
    if M >= 2:
        assert kept < peaks
    if M >= 3 and family == "tie":
        assert ties > 0
    assert same_bits(want[:, M:], maps[:, M:])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_nms_equals_the_definition(shape, family, layout):
    B, M, N, h, w, R = shape
    x, maps, want = reference(shape, family)
    P = maps[:, :M]
    got = run_label_nms(lay_out(P, layout), R, offset_out=layout == "offset")
    assert same_bits(got, expected_label_nms(P, R))
    assert same_bits(got, want[:, :M])


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_nms_of_the_nms5_output_is_the_plain_path(shape, family):
    """What `LabelNms` does around the bare network: `sd_nms5` with the sigmoid fused over the M + N channels, then `sd_label_nms` on the
    label channels of ITS output, a channel-slice view; the part channels stay `sd_nms5`'s."""
    B, M, N, h, w, R = shape
    x, maps, want = reference(shape, family)
    got = nms5_sigmoid(x)
    assert same_bits(got, maps)
    assert same_bits(run_label_nms(got[:, :M], R), want[:, :M])


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("h,w", [(8, 12), (33, 70), (128, 128)])
def test_one_label_within_the_5x5_window_is_the_identity(h, w, R):
    x = normal_logits((2, 3, h, w), 7 * h + R, "cuda")              # distinct values: a 9x9 window always thins the 5x5 peaks
    maps = nms5_sigmoid(x)
    for c in range(3):
        assert same_bits(run_label_nms(maps[:, c:c + 1], R), maps[:, c:c + 1])
    wide = run_label_nms(maps[:, :1], 4)
    assert not torch.equal(wide, maps[:, :1]) and same_bits(wide, expected_label_nms(maps[:, :1], 4))


def planted(M, N, h, w, peaks):
    """Logits of -9 everywhere but at the (channel, y, x, logit) peaks, their probabilities, and what the plain path makes of them:
    `sd_label_nms` at radius R of the label channels of `sd_nms5`'s output."""
    from structuredetector_amd.utils.ops import clamped_sigmoid
    x = torch.full((1, M + N, h, w), -9.0, device="cuda")
    for c, y, xx, v in peaks:
        x[0, c, y, xx] = v
    return x, clamped_sigmoid(x), lambda R: run_label_nms(nms5_sigmoid(x)[:, :M], R)


@pytest.mark.parametrize("R", [2, 4, 8])
@pytest.mark.parametrize("axis", ["x", "y", "diagonal"])
def test_planted_neighbours_keep_the_higher_label_up_to_R_cells(R, axis):
    """Two labels k cells apart: only the higher survives for k <= R, both for k = R + 1 (across a tile border: the pair straddles column
    64 / row 16)."""
    h, w = 40, 136
    for k in range(1, R + 2):
        y0, x0 = 15 - (k // 2 if axis != "x" else 0), 63 - (k // 2 if axis != "y" else 0)
        y1, x1 = y0 + (k if axis != "x" else 0), x0 + (k if axis != "y" else 0)
        x, p, run = planted(2, 1, h, w, [(1, y0, x0, 2.0), (0, y1, x1, 1.0)])
        got = run(R)
        assert got[0, 1, y0, x0] == p[0, 1, y0, x0] and got[0, 0, y0, x0] == 0
        assert got[0, 0, y1, x1] == (p[0, 0, y1, x1] if k == R + 1 else 0), (k, R)
        assert got[0, 1, y1, x1] == 0
        assert same_bits(got, expected_nms5_labels(x, 2, R)[:, :2])


def test_planted_ties_and_corners():
    R = 2
    # equal logits under two labels at one cell: the lower label keeps the peak
    x, p, run = planted(3, 1, 20, 70, [(1, 9, 65, 1.5), (2, 9, 65, 1.5)])
    got = run(R)
    assert got[0, 1, 9, 65] == p[0, 1, 9, 65] and got[0, 2, 9, 65] == 0 and got[0, 0, 9, 65] == 0
    assert same_bits(got, expected_nms5_labels(x, 3, R)[:, :3])
    # equal logits at two cells within R, under two labels: both survive
    x, p, run = planted(2, 1, 20, 70, [(0, 9, 63, 1.5), (1, 10, 65, 1.5)])
    got = run(R)
    assert got[0, 0, 9, 63] == p[0, 0, 9, 63] and got[0, 1, 10, 65] == p[0, 1, 10, 65]
    assert same_bits(got, expected_nms5_labels(x, 2, R)[:, :2])
    # peaks in the four corners of a map see no padding, at the largest radius
    h, w = 17, 66
    x, p, run = planted(2, 1, h, w, [(1, 0, 0, -8.5), (0, 0, w - 1, -8.5), (1, h - 1, 0, -8.5), (0, h - 1, w - 1, -8.5)])
    got = run(8)
    for c, y, xx in ((1, 0, 0), (0, 0, w - 1), (1, h - 1, 0), (0, h - 1, w - 1)):
        assert got[0, c, y, xx] == p[0, c, y, xx] > 0
    assert same_bits(got, expected_nms5_labels(x, 2, 8)[:, :2])


def test_python_wrapper_takes_views_without_a_copy():
    from structuredetector_amd.model.label_nms import label_nms, nms5_sigmoid as wrapped_nms5
    shape = SHAPES[3]
    B, M, N, h, w, R = shape
    x, maps, want = reference(shape, "tie")
    head = torch.cat([x, torch.zeros(B, 4, h, w, device="cuda")], 1)
    assert same_bits(wrapped_nms5(head[:, :M + N]), maps)
    assert same_bits(label_nms(maps[:, :M], R), want[:, :M])
