"""Memory guards of the tests that call the library straight at the C ABI (tests/test_gpu_gemm_small_abi.py,
tests/test_gpu_gemm_pair_abi.py, tests/test_gpu_wino7_abi.py, tests/test_gpu_mask_iou_abi.py, tests/test_gpu_image_prep_abi.py,
tests/test_gpu_pool.py): operands inside NaN-poisoned memory, outputs inside sentinel memory, pair images a kernel writes inside
fp16 NaN, a split-K workspace that is NaN until it is written, the bit-for-bit comparison that names the first wrong element, and
the integer variants: byte operands inside 0xFF, integer results inside a sentinel of their type."""
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

    def check(self, finite=True):
        """Everything inside [M][N] finite (finite = False: merely no longer the sentinel's bits, for results that may be
        infinite), everything outside untouched (compared as int32). -> the dense result"""
        got = self.view.clone()
        if finite:
            assert bool(torch.isfinite(got).all()), "an element of the result was not written (or is not finite)"
        else:
            assert bool((got.view(torch.int32) != SENT).all()), "an element of the result was not written"
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


# ---- integer buffers: masks and images (uint8), half maps as their bits (uint16), areas and arg-max (int32), packed words (int64) ----

SENT_U8 = 0xFF               # the byte poison: a read past a mask's row or past the last mask turns bits ON
SENT_U16 = 0x7BFF            # 65504, the largest finite half: no ratio of two counts and not a NaN
SENT_I32 = -0x41105EA1       # no count and no arg-max is negative
SENT_I64 = 0x5EA15EA15EA15EA1
_INT_SENT = {torch.uint8: SENT_U8, torch.int16: SENT_U16, torch.int32: SENT_I32, torch.int64: SENT_I64}


class _OutInt:
    """_Out for integer results: [M][N] of `dtype` (uint8, int16 for the bits of a uint16, int32, int64) with leading dimension
    N + pad, two guard rows + 64 elements on either side, every element preset to the dtype's sentinel above."""

    def __init__(self, M, N, pad, dev, dtype):
        self.M, self.N, self.ld, self.sent = M, N, N + pad, _INT_SENT[dtype]
        self.front = (2 * self.ld + GUARD + 15) // 16 * 16
        total = self.front + M * self.ld + 2 * self.ld + GUARD
        self.raw = torch.full((total,), self.sent, dtype=dtype, device=dev)
        self.view = self.raw.as_strided((M, N), (self.ld, 1), self.front)
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == 0

    def untouched(self):
        return bool((self.raw == self.sent).all())

    def check(self):
        """Every element inside [M][N] written (no longer the sentinel), everything outside untouched. -> the dense result"""
        got = self.view.clone()
        left = int((got == self.sent).sum())
        assert left == 0, "%d elements of the result were not written, the first at %s" % (left, (got == self.sent).nonzero()[0].tolist())
        rest = self.raw.clone()
        rest.as_strided((self.M, self.N), (self.ld, 1), self.front).fill_(self.sent)
        assert bool((rest == self.sent).all()), "a store outside [M][N]: %d elements changed" % int((rest != self.sent).sum())
        return got


def _poisoned_u8(t, shift=0, front=None, back=None):
    """The bytes of the dense uint8 tensor `t` inside a poisoned buffer, 64 + shift bytes in front (shift = 0: the first byte is
    16-byte aligned; 1: aligned to nothing) and 64 behind.  The poison is 0xFF, or the byte patterns `front` / `back` (uint8
    tensors that are repeated towards the outside, front's last byte lying just before the data).  -> the view"""
    n = t.numel()
    lead = GUARD + shift
    buf = torch.full((lead + n + GUARD,), SENT_U8, dtype=torch.uint8, device=t.device)
    if front is not None:
        reps = (lead + front.numel() - 1) // front.numel()
        buf[:lead] = front.repeat(reps)[-lead:]
    if back is not None:
        buf[lead + n:] = back.repeat((GUARD + back.numel() - 1) // back.numel())[:GUARD]
    v = buf[lead:lead + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == shift
    return v


def _poisoned_i64(t):
    """The values of the dense int64 tensor `t` with 64 words of all-ones on either side (a read past the packed masks adds set
    bits to a count).  -> the view"""
    buf = torch.full((GUARD + t.numel() + GUARD,), -1, dtype=torch.int64, device=t.device)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v
