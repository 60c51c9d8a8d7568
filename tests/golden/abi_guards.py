"""Memory guards of the tests that call the library straight at the C ABI (tests/test_gpu_gemm_small_abi.py,
tests/test_gpu_gemm_pair_abi.py, tests/test_gpu_wino7_abi.py): operands inside NaN-poisoned memory, outputs inside sentinel memory,
pair images a kernel writes inside fp16 NaN, a split-K workspace that is NaN until it is written, and the bit-for-bit comparison
that names the first wrong element."""
import torch

NAN = float("nan")
SENT = 0x7FC0BEEF        # the bit pattern every output float holds before a call (a quiet NaN: an unwritten result is not finite)
GUARD = 64               # floats of poison / sentinel around every buffer


def _poisoned(t, pad=0):
    """The [rows][cols] values of `t` (cols contiguous) with leading dimension cols + pad inside a NaN-filled buffer: 65 NaN floats
    in front (odd: the base is 4-byte aligned and no more), NaN in every gap, 64 behind the last element.  -> (view, ld)"""
    rows, cols = t.shape
    ld = cols + pad
    front = GUARD + 1
    buf = torch.full((front + (rows - 1) * ld + cols + GUARD,), NAN, dtype=torch.float32, device=t.device)
    v = buf.as_strided((rows, cols), (ld, 1), front)
    v.copy_(t)
    assert v.data_ptr() % 8 == 4
    return v, ld


def _poisoned16(t):
    """The values of the dense tensor `t` (any shape) inside a NaN-filled buffer, 64 NaN floats on either side, the first element
    16-byte aligned: for the kernels that read their operand as float4.  -> the view"""
    buf = torch.full((GUARD + t.numel() + GUARD,), NAN, dtype=torch.float32, device=t.device)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return v


F16_NAN2 = 0x7E007E00        # two fp16 quiet NaNs: what every int32 of a pair-image buffer holds before a call


class _ImageOut:
    """A pair image of n int32 that a kernel is to write, 32-byte aligned, preset to fp16 NaN like the 64 int32 on either side."""

    def __init__(self, n, dev):
        self.n = n
        self.raw = torch.full((GUARD + n + GUARD,), F16_NAN2, dtype=torch.int32, device=dev)
        self.ptr = self.raw.data_ptr() + 4 * GUARD
        assert self.ptr % 32 == 0

    def check(self):
        """Everything outside the n words unchanged, every word inside written. -> the image, int32 [n] on the host"""
        raw = self.raw.cpu().numpy()
        out = (raw[:GUARD] != F16_NAN2).sum() + (raw[GUARD + self.n:] != F16_NAN2).sum()
        assert out == 0, "a store outside the image: %d int32 changed" % int(out)
        img = raw[GUARD:GUARD + self.n]
        left = int((img == F16_NAN2).sum())
        assert left == 0, "%d int32 of the image were not written, the first at %d" % (left, int((img == F16_NAN2).argmax()))
        return img


class _Out:
    """An [M][N] output with leading dimension N + pad, two guard rows + 64 floats on either side, every float preset to SENT.
    shift = 0: the first element is 16-byte aligned; shift = 1: 4-byte aligned only."""

    def __init__(self, M, N, pad, dev, shift=1):
        self.M, self.N, self.ld = M, N, N + pad
        self.front = (2 * self.ld + GUARD + 3) // 4 * 4 + shift
        total = self.front + M * self.ld + 2 * self.ld + GUARD
        self.raw = torch.full((total,), SENT, dtype=torch.int32, device=dev)
        self.view = self.raw.view(torch.float32).as_strided((M, N), (self.ld, 1), self.front)
        self.ptr = self.view.data_ptr()
        assert self.raw.data_ptr() % 16 == 0 and self.ptr % 16 == 4 * shift

    def check(self):
        """Everything inside [M][N] finite, everything outside untouched (compared as int32). -> the dense result"""
        got = self.view.clone()
        assert bool(torch.isfinite(got).all()), "an element of the result was not written (or is not finite)"
        rest = self.raw.clone()
        rest.as_strided((self.M, self.N), (self.ld, 1), self.front).fill_(SENT)
        assert bool((rest == SENT).all()), "a store outside [M][N]: %d floats changed" % int((rest != SENT).sum())
        return got


class _Ws:
    """A split-K workspace of exactly n floats, pre-filled with NaN (a partial that is read before it is written shows in the
    result), between sentinel floats.  shift as _Out."""

    def __init__(self, n, dev, shift=1):
        self.n, self.front = n, GUARD + shift
        self.raw = torch.full((self.front + n + GUARD,), SENT, dtype=torch.int32, device=dev)
        self.raw[self.front:self.front + n].view(torch.float32).fill_(NAN)
        self.ptr = self.raw.data_ptr() + 4 * self.front
        assert self.ptr % 16 == 4 * shift

    def check(self):
        assert bool((self.raw[:self.front] == SENT).all()) and bool((self.raw[self.front + self.n:] == SENT).all()), \
            "a store outside the workspace's splits * M * N floats"


def _same(got, want, what):
    """Bit-for-bit agreement of a float32 result with the float64 reference of integer data."""
    want = want.to(got.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        first = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.numel(), first, float(got[tuple(first)]), float(want[tuple(first)])))
