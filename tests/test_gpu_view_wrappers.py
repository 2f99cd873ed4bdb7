"""The wrappers around `net` (`FlipTta`, `ScaleTta`, `TransposeTta`, `TiledNet`) on a stub `net`, in every form a forward's output can
take: whether the heatmaps arrive as one raw head tensor, as adjacent channel slices of one (ONE merge launch over the M + N channels)
or as tensors of their own (TWO launches, on the anchor and on the part maps), the result is the same, bit for bit."""
import pytest
import torch

from tests.test_gpu_tta import default_label_args

pytestmark = pytest.mark.gpu

B = 2


class StubNet:
    """A callable in place of a `Network`: random head logits of the right shape for its input, seeded by the input's shape, returned as
      "a": the raw head tensor;   "b": the dict of its four channel-slice views;   "c": the same dict, every tensor a clone of its own.
    config: one of the three, or {(H, W) of the input: one of the three}.  `heads` keeps the head tensor of every call."""

    def __init__(self, args, config):
        self.M, self.nb = len(args.labels), len(args.labels) + len(args.parts)
        self.config, self.heads = config, []

    def __call__(self, x):
        n, _, H, W = x.shape
        gen = torch.Generator("cuda").manual_seed((n * 4099 + H) * 4099 + W)
        head = torch.randn(n, self.nb + 4, H // 4, W // 4, device="cuda", generator=gen) * 3
        self.heads.append(head)
        config = self.config if isinstance(self.config, str) else self.config[(H, W)]
        if config == "a":
            return head
        M, nb = self.M, self.nb
        out = {"anchor_hm": head[:, :M], "part_hm": head[:, M:nb], "offsets": head[:, nb:nb + 2], "embeddings": head[:, nb + 2:nb + 4]}
        return out if config == "b" else {k: v.clone() for k, v in out.items()}


def images_at(size):
    """The same random (B, 3, H, W) batch for every call with one (width, height)."""
    gen = torch.Generator("cuda").manual_seed(size[0] * 4099 + size[1])
    return torch.randn(B, 3, size[1], size[0], device="cuda", generator=gen)


def check(wrap, H, W, configs, views_of_the_head=True):
    """wrap(net) -> the wrapper's call on the (B, 3, H, W) batch.  Every configuration gives the same four maps; in "a" and "b" the
    regressions are views into the head tensor of the stub's first forward (the one that held view 0)."""
    args = default_label_args(width=W, height=H)
    M, N = len(args.labels), len(args.parts)
    x = images_at((W, H))
    first = None
    for config in configs:
        net = StubNet(args, config)
        got = wrap(net, args)(x)
        assert set(got) == {"anchor_hm", "part_hm", "offsets", "embeddings"}
        assert got["anchor_hm"].shape[:2] == (B, M) and got["part_hm"].shape[:2] == (B, N)
        if views_of_the_head and config in ("a", "b"):
            for k in ("offsets", "embeddings"):
                assert got[k].untyped_storage().data_ptr() == net.heads[0].untyped_storage().data_ptr(), (config, k)
        if first is None:
            first = got
        for k in first:
            assert got[k].shape == first[k].shape and torch.equal(got[k], first[k]), (config, k)
    assert first["anchor_hm"].count_nonzero() > 0 and first["part_hm"].count_nonzero() > 0


SHAPES = [(32, 32), (32, 64)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_flip_tta_in_every_output_form(H, W):
    from structuredetector_amd.model.tta import FlipTta
    check(lambda net, args: FlipTta(net, args, "hvflip"), H, W, ["a", "b", "c"])


@pytest.mark.parametrize("mode", ["none", "hflip"])
def test_scale_tta_in_every_output_form(mode):
    from structuredetector_amd.model.tta import ScaleTta
    sizes = [(32, 32), (64, 64)]
    check(lambda net, args: (lambda x: ScaleTta(net, args, sizes, mode)(x, at_size=images_at)), 32, 32,
          ["a", "b", "c", {(32, 32): "b", (64, 64): "c"}])


@pytest.mark.parametrize("H,W", SHAPES)
def test_transpose_tta_in_every_output_form(H, W):
    from structuredetector_amd.model.tta import TransposeTta
    mixed = [{(H, W): "b", (W, H): "c"}] if H != W else []             # the plain forward one launch's form, the transposed one the other's
    check(lambda net, args: TransposeTta(net, args, "hflip"), H, W, ["a", "b", "c"] + mixed)


@pytest.mark.parametrize("H,W", SHAPES)
def test_tiled_net_in_every_output_form(H, W):
    """2 x 1 tiles with overlap 0: the smallest grid that stitches, and the only overlap a 32-pixel side admits.  The regressions are the
    merge launch's own output (the owner tiles' copies), so they are compared, not traced to the head tensor."""
    from structuredetector_amd.model.tiles import TiledNet
    check(lambda net, args: (lambda x: TiledNet(net, args, (2, 1), 0)(x, at_size=images_at)), H, W, ["a", "b", "c"], views_of_the_head=False)
