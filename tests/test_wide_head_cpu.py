"""Wide heads (33 .. 256 output channels = up to 252 labels + parts): construction limits of `Network` and the host-side checks of the
head entry points.  No GPU needed: nothing here launches a kernel."""
from argparse import Namespace

import pytest

SD_ERR_INVALID, SD_ERR_WORKSPACE, SD_ERR_ALIGN = -1, -2, -3          # include/sdnet_hip.h


def _args(M, N, fpn_depth=128):
    return Namespace(labels={f"l{i}": i for i in range(M)}, parts={f"p{i}": i for i in range(N)}, fpn_depth=fpn_depth)


def test_wide_head_constructs():
    from structuredetector_amd.model import Network
    net = Network(_args(30, 20), pretrained=False)
    assert net.out_channels == 54
    assert tuple(net.head.conv.weight.shape) == (54, 128, 1, 1) and tuple(net.head.conv.bias.shape) == (54,)


@pytest.mark.parametrize("fpn_depth", [64, 128, 256])
def test_widest_head_constructs(fpn_depth):
    from structuredetector_amd.model import Network
    net = Network(_args(200, 52, fpn_depth), pretrained=False)
    assert tuple(net.head.conv.weight.shape) == (256, fpn_depth, 1, 1)


def test_head_wider_than_256_raises():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    with pytest.raises(L.SdError, match="256"):
        Network(_args(200, 53), pretrained=False)


def test_wide_head_needs_a_supported_fpn_depth():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    with pytest.raises(L.SdError, match="fpn_depth"):
        Network(_args(30, 20, fpn_depth=192), pretrained=False)
    Network(_args(20, 8, fpn_depth=192), pretrained=False)        # 32 channels: the narrow kernels, any multiple of 64


def test_wide_head_workspace_is_bounded_and_narrow_sizes_unchanged():
    """sd_head_bwd_workspace_bytes: the narrow formula for Co <= 32 (max(blocks of 1024 pixels, waves of 16-pixel tiles up to 1024) partial
    rows of Co * C + Co floats, 256-byte aligned), at most 64 MB for every wide shape up to bs = 64 at 512 x 512."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    for B, HW, C, Co in [(64, 128 * 128, 128, 7), (2, 60, 128, 7), (1, 1665, 64, 32), (64, 128 * 128, 256, 32)]:
        M = B * HW
        rows = max(-(-M // 1024), min(1024, (-(-M // 16) + 3) // 4 * 4))
        want = -(-rows * (Co * C + Co) * 4 // 256) * 256
        assert lib.sd_head_bwd_workspace_bytes(B, HW, C, Co) == want
    for C in (64, 128, 256):
        for Co in (33, 64, 65, 100, 132, 200, 256):
            for B, HW in [(64, 128 * 128), (1, 1665), (2, 48 * 48)]:
                n = lib.sd_head_bwd_workspace_bytes(B, HW, C, Co)
                assert (Co * C + Co) * 4 <= n <= 64 << 20, (B, HW, C, Co, n)


def test_wide_head_rejects_unsupported_shapes_before_launch():
    """Unsupported wide shapes come back as SD_ERR_INVALID from the host-side checks (the pointers are never dereferenced)."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    p = 4096                                                   # 16-byte aligned, never touched
    assert lib.sd_head_fwd(p, p, p, p, 1, 64, 96, 40, None) == SD_ERR_INVALID
    assert lib.sd_head_fwd_bf16(p, p, p, p, 1, 64, 96, 40, None) == SD_ERR_INVALID
    assert lib.sd_head_fwd(p, p, p, p, 1, 64, 128, 257, None) == SD_ERR_INVALID
    assert lib.sd_head_fwd(p, p, p, p, 1 << 15, 1 << 16, 128, 64, None) == SD_ERR_INVALID      # B * HW = 2^31
    assert lib.sd_head_fwd(p + 4, p, p, p, 1, 64, 128, 64, None) == SD_ERR_ALIGN
    assert lib.sd_head_fwd_bf16(p + 8, p, p, p, 1, 64, 128, 64, None) == SD_ERR_ALIGN
    ws = lib.sd_head_bwd_workspace_bytes(1, 64, 96, 40)
    assert lib.sd_head_bwd(p, p, p, p, p, p, 1, 64, 96, 40, 0, p, ws, None) == SD_ERR_INVALID
    ws = lib.sd_head_bwd_workspace_bytes(1, 64, 128, 64)
    assert lib.sd_head_bwd(p, p, p, p, p, p, 1, 64, 128, 64, 0, p, ws - 1, None) == SD_ERR_WORKSPACE
