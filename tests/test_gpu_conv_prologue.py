"""GPU: the index prologue of the fp32 conv tiles after it moved to host-made division constants (csrc/fastdiv.h) and one fetched
prologue block (csrc/conv_f32_common.h: ConvPro).  Every quotient the kernels used to form with `/` - workgroup -> (k-slice, group,
tile), tile -> (channel block, pixel block), the split-K bounds, k-tile -> (tap, chunk), row -> (image, pixel), pixel -> (oh, ow),
tap -> (kh, kw) - takes several values and leaves a remainder in the cases below, the smallest that do so; the problem selection
by start[] is covered by a batch of four different geometries, and xcd_remap's remainder branch by a block count above 8 that is
no multiple of 8.  Operands are small integers, so every sum is exact in float32 and the comparison with the float64 reference is
torch.equal.  Tiles: the frame's 32 x 64 and 32 x 32 producer / consumer tiles (55, 53) and its v2 32 x 64 tile (14)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
V3_64, V3_32, V2_64 = 55, 53, 14
TILES = [V3_64, V3_32, V2_64]
SENT = -12345.0
EINVAL = -1


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


class Prob:
    """one convolution with integer operands: device buffers (y between guard rows, all prefilled with SENT) and the float64 result"""

    def __init__(self, seed, N, H, W, Cin, Cout, k=3, stride=1, pad=0, dil=1, groups=1, relu=True, bias=True):
        self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.stride, self.pad, self.dil, self.G = N, H, W, Cin, Cout, k, stride, pad, dil, groups
        self.relu = relu
        x = ints((groups, N, Cin, H, W), -3, 3, seed)
        w = ints((groups, Cout, Cin, k, k), -2, 2, seed + 1)
        b = ints((groups, Cout), -9, 9, seed + 2) if bias else torch.zeros(groups, Cout)
        ref = torch.stack([F.conv2d(x[g].double(), w[g].double(), b[g].double(), stride=stride, padding=pad, dilation=dil) for g in range(groups)])
        self.raw64 = (ref - b.double()[:, None, :, None, None]).permute(0, 1, 3, 4, 2).contiguous()      # [G][N][OH][OW][Cout], no bias
        if relu:
            ref = ref.relu()
        self.ref = ref.permute(0, 1, 3, 4, 2).contiguous()
        self.OH, self.OW = ref.shape[3], ref.shape[4]
        self.M = N * self.OH * self.OW
        self.K = k * k * Cin
        self.x = x.permute(0, 1, 3, 4, 2).contiguous().to(DEV)                                          # [G] NHWC
        self.w = w.permute(0, 1, 3, 4, 2).reshape(groups, Cout, self.K).contiguous().to(DEV)             # k = (kh KW + kw) Cin + ci
        self.b = b.to(DEV)
        self.ybuf = torch.full((groups * self.M * Cout + 2 * 256,), SENT, device=DEV)
        self.y = self.ybuf[256:256 + groups * self.M * Cout].view(groups, N, self.OH, self.OW, Cout)
        self.ws = None

    def desc(self, tile, ksplit=1, defer=0, n_dyn=None, n_first=0):
        self.tick = 0
        if ksplit > 1:
            self.tick = ksplit * self.G * self.M * self.Cout
            self.ws = torch.full((self.tick + self.G * ((self.M + 15) // 16) * ((self.Cout + 31) // 32),), SENT, device=DEV)
            self.ws[self.tick:].zero_()
        return hip.conv_desc(self.x.data_ptr(), self.w.data_ptr(), self.b.data_ptr(), self.y.data_ptr(), N=self.N, H=self.H, W=self.W,
                             Cin=self.Cin, OH=self.OH, OW=self.OW, Cout=self.Cout, KH=self.k, KW=self.k, stride=self.stride,
                             pad=(self.pad, self.pad), dil=(self.dil, self.dil), act=hip.ACT_RELU if self.relu else hip.ACT_NONE,
                             groups=self.G, x_gs=self.N * self.H * self.W * self.Cin, w_gs=self.Cout * self.K, b_gs=self.Cout,
                             y_gs=self.M * self.Cout, tile=tile, ksplit=ksplit, defer=defer,
                             ws=self.ws.data_ptr() if self.ws is not None else None, n_dyn=n_dyn, n_first=n_first)

    def guards_intact(self):
        return bool((self.ybuf[:256] == SENT).all()) and bool((self.ybuf[-256:] == SENT).all())

    def check(self, what):
        assert self.guards_intact(), what
        got = self.y.cpu().double()
        assert torch.equal(got, self.ref), (what, int((got != self.ref).sum()), 'of', got.numel())
        if self.ws is not None:
            assert not bool(self.ws[self.tick:].view(torch.int32).any()), (what, 'ticket words')


def launch(descs):
    arr = (hip.ConvDesc * len(descs))(*descs)
    rc = hip.lib().usot_conv2d_batch_f32(hip.stream(), arr, len(descs))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('tile', TILES)
def test_four_problems_of_different_geometry_in_one_launch(tile):
    ps = [Prob(10, 2, 5, 5, 64, 80, pad=1), Prob(20, 1, 7, 3, 64, 80, pad=1), Prob(30, 1, 7, 7, 64, 80, stride=2), Prob(40, 1, 6, 6, 64, 80, pad=2, dil=2)]
    assert [(p.OH, p.OW) for p in ps] == [(5, 5), (7, 3), (3, 3), (6, 6)]
    assert launch([p.desc(tile) for p in ps]) == 0
    for i, p in enumerate(ps):
        p.check('tile %d problem %d' % (tile, i))


@pytest.mark.parametrize('ksplit', [2, 3])
@pytest.mark.parametrize('tile', TILES)
def test_groups_and_uneven_split_k(tile, ksplit):
    """groups = 3, K = 576: nine k-tiles of 64 (eighteen of 32 on the v2 tile) in 2 or 3 slices; combined in the launch, and as the
    deferred partial tiles [ksplit][groups][M][Cout] (no bias, no activation) summed here"""
    p = Prob(50 + ksplit, 1, 5, 5, 64, 40, pad=1, groups=3)
    assert p.K == 576
    assert launch([p.desc(tile, ksplit=ksplit)]) == 0
    p.check('combine, tile %d ksplit %d' % (tile, ksplit))
    q = Prob(50 + ksplit, 1, 5, 5, 64, 40, pad=1, groups=3)
    assert launch([q.desc(tile, ksplit=ksplit, defer=1)]) == 0
    assert q.guards_intact() and bool((q.ybuf == SENT).all())                        # a deferred launch does not write y
    parts = q.ws[:q.tick].view(ksplit, 3, 1, 5, 5, 40).cpu().double()
    assert torch.equal(parts.sum(0), q.raw64), (tile, ksplit)
    assert bool((parts != 0).flatten(1).any(1).all())                                # every slice carried part of the sum


@pytest.mark.parametrize('tile', TILES)
def test_two_chunks_per_tap_split_inside_a_tap(tile):
    """Cin = 128: k-tile -> (tap, chunk) and tap -> (kh, kw) change inside one k-slice; 18 k-tiles of 64 in two slices of nine,
    the second of which starts at chunk 1 of tap 4"""
    p = Prob(70, 1, 5, 5, 128, 40, pad=1)
    assert launch([p.desc(tile, ksplit=2)]) == 0
    p.check('tile %d' % tile)


@pytest.mark.parametrize('count', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('tile', [V3_64, V3_32])
def test_run_time_image_count(tile, count):
    """n_dyn with N = 3 images of 5 x 5 and n_first = 1: clamp(count - 1, 0, 3) images are live, the rows past them keep the prefill"""
    p = Prob(80, 3, 5, 5, 64, 80, pad=1)
    word = torch.tensor([count], dtype=torch.int32, device=DEV)
    assert launch([p.desc(tile, n_dyn=word.data_ptr(), n_first=1)]) == 0
    live = min(max(count - 1, 0), 3)
    assert p.guards_intact()
    got = p.y.cpu().double()
    assert torch.equal(got[0, :live], p.ref[0, :live]), (tile, count)
    assert bool((got[0, live:] == SENT).all()), (tile, count)


@pytest.mark.parametrize('tile', TILES)
def test_block_count_above_eight_and_no_multiple_of_eight(tile):
    """1 x 1, M = 121, Cout = 160: 4 x 3 = 12 workgroups on the 32 x 64 tiles, 4 x 5 = 20 on the 32 x 32 tile - xcd_remap's remainder
    branch (total & 7 = 4) - and tile -> (channel block, pixel block) with a quotient above 1 and a remainder"""
    bm, bn = hip.tile_table()[tile]
    p = Prob(90, 1, 11, 11, 64, 160, k=1)
    blocks = -(-p.M // bm) * -(-p.Cout // bn)
    assert blocks > 8 and blocks % 8 != 0, blocks
    assert launch([p.desc(tile)]) == 0
    p.check('tile %d' % tile)


@pytest.mark.parametrize('tile', TILES)
def test_a_problem_beyond_the_dividend_range_is_refused(tile):
    """N x OH x OW = 2^22 x 23 x 23 > 2^31 - 1 rows: outside the range fastdiv.h is proven for; USOT_EINVAL before anything is
    launched (the buffers are those of a one-image problem: nothing may be read or written)"""
    p = Prob(95, 1, 23, 23, 64, 64, k=1)
    d = p.desc(tile)
    d.N = 1 << 22
    assert launch([d]) == EINVAL
    assert bool((p.ybuf == SENT).all())
    d.N = 1
    assert launch([d]) == 0                                                          # the same descriptor inside the range runs
    p.check('tile %d' % tile)
