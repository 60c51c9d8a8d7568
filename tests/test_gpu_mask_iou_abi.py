"""-m gpu: cim_mask_pack and cim_mask_iou_pair (cim_amd/csrc/mask_iou.hip) straight at the C ABI against tests/golden/mask_cases.py,
the NumPy statement of the packing and of the maps that tests/test_mask_cases_cpu.py holds to the oracle.

Every comparison is exact: packed words as integers, areas as integers, the two half maps as their 16 bits wherever the
reference is not NaN.  Where it is NaN (0 / 0: an empty mask's diagonal, its column of asy, two empty masks) the device must give a
NaN too; sign and payload are not compared (the host's 0 / 0 is 0xFE00, the device's pattern is printed by the pair test).

Guards on every call (tests/golden/abi_guards.py): masks inside 0xFF bytes (a read past a row or past the last mask turns tail
bits on), packed words inside all-ones words, every result inside sentinel memory (written everywhere inside, untouched
outside); the sentinel of `area` doubles as the garbage the call has to clear before its atomics.

Shapes come from the kernels' own tiling: the 16-byte pack kernel's split inside a word (HW = 12, 60, 68), its chunk of 1024 pixels
(1020 .. 1040) and a last chunk of one word (1028, 1040, 2052), each HW % 4 == 0 also from a base one byte off (the scalar
kernel); the pair kernel's 64-mask tiles (N = 63 .. 65, 128, 129, 193: mirrored tiles of one row) and its 32-word LDS stage
(words = 1, 31, 32, 33, 65)."""
import numpy as np
import pytest
import torch

import mask_cases as mc
from abi_guards import _OutInt, _poisoned_i64, _poisoned_u8      # tests/golden/abi_guards.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _words_dev(dev, words_u64):
    return torch.from_numpy(np.ascontiguousarray(words_u64).view(np.int64)).to(dev)


# ---- cim_mask_pack ---------------------------------------------------------------------------------------------------------------

def _pack(dev, m, shift):
    """m uint8 [N, HW] through cim_mask_pack from a base `shift` bytes past a 16-byte boundary -> [words, N] uint64 on the host"""
    from cim_amd import _lib
    n, hw = m.shape
    md = _poisoned_u8(torch.from_numpy(m).to(dev), shift=shift)
    out = _OutInt(mc.n_words(hw), n, 0, dev, torch.int64)
    _lib.call("cim_mask_pack", md.data_ptr(), out.ptr, n, hw, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.check().cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("hw", [1, 3, 4, 12, 16, 60, 63, 64, 65, 68, 1020, 1023, 1024, 1028, 1040, 2052])
def test_pack_equals_the_definition(dev, hw):
    for n in (1, 3, 65):
        m = mc.byte_masks(n, hw)
        m[n - 1, hw - 1] = 0x80                                          # the last pixel of the last mask is set
        want = mc.pack_words(m)
        got = _pack(dev, m, 0)
        assert np.array_equal(got, want), (n, hw, np.argwhere(got != want)[:4].tolist())
        assert not mc.unpack_words(got)[:, hw:].any(), "tail bits set"
        if hw % 4 == 0:                                                  # the same bytes, one byte off: the scalar kernel
            again = _pack(dev, m, 1)
            assert np.array_equal(again, got), (n, hw, np.argwhere(again != got)[:4].tolist())


def test_pack_small_named_masks(dev):
    m, _ = mc.small_masks()
    for cols in (130, 128):                                              # the scalar kernel, the 16-byte kernel
        sub = np.ascontiguousarray(m[:, :cols])
        assert np.array_equal(_pack(dev, sub, 0), mc.pack_words(sub))


# ---- cim_mask_iou_pair -----------------------------------------------------------------------------------------------------------

def _nan16(bits):
    return (bits & 0x7FFF) > 0x7C00


def _same_map(got_bits, want_f16, what):
    want = want_f16.view(np.uint16)
    nan = np.isnan(want_f16)
    assert np.array_equal(_nan16(got_bits), nan), "%s: NaN positions differ at %s" % (what, np.argwhere(_nan16(got_bits) != nan)[:4].tolist())
    bad = (got_bits != want) & ~nan
    assert not bad.any(), "%s: %d entries differ, first at %s: got 0x%04x, want 0x%04x" % (
        what, int(bad.sum()), np.argwhere(bad)[0].tolist(), got_bits[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


class _PairCall:
    """One set of guarded buffers of cim_mask_iou_pair; run() may be repeated on them"""

    def __init__(self, dev, words_u64):
        self.words, self.n = words_u64.shape
        self.packed = _poisoned_i64(_words_dev(dev, words_u64))
        self.area = _OutInt(1, self.n, 0, dev, torch.int32)              # its sentinel is the garbage the call must clear
        self.iou = _OutInt(self.n, self.n, 0, dev, torch.int16)
        self.asy = _OutInt(self.n, self.n, 0, dev, torch.int16)

    def run(self):
        from cim_amd import _lib
        _lib.call("cim_mask_iou_pair", self.packed.data_ptr(), self.n, self.words, self.area.ptr, self.iou.ptr, self.asy.ptr,
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        return (self.iou.check().cpu().numpy().view(np.uint16), self.asy.check().cpu().numpy().view(np.uint16),
                self.area.check().cpu().numpy().reshape(self.n))


def _pair_case(dev, words_u64, what):
    call = _PairCall(dev, words_u64)
    iou, asy, area = call.run()
    riou, rasy, rarea = mc.maps_from_words(words_u64)
    assert np.array_equal(area.astype(np.int64), rarea), "%s: area differs from the popcount at %s" % (
        what, np.flatnonzero(area != rarea)[:4].tolist())
    _same_map(iou, riou, what + " iou")
    _same_map(asy, rasy, what + " asy")
    nan = _nan16(iou)
    assert np.array_equal(nan, nan.T) and np.array_equal(iou[~nan], iou.T[~nan]), what + ": iou is not its transpose"
    iou2, asy2, area2 = call.run()                                       # the same buffers again: area is cleared by the call itself
    assert np.array_equal(iou2, iou) and np.array_equal(asy2, asy) and np.array_equal(area2, area), what + ": a second call differs"
    return iou, asy


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 193])
def test_pair_maps_equal_the_definition(dev, n):
    nans = set()
    for words in (1, 31, 32, 33, 65):
        iou, asy = _pair_case(dev, mc.pair_words(n, words), "N = %d, words = %d" % (n, words))
        nans |= set(iou[_nan16(iou)].tolist()) | set(asy[_nan16(asy)].tolist())
    print("N = %d: the device's NaN bits: %s (the host's 0 / 0 is 0xfe00)" % (n, sorted("0x%04x" % v for v in nans)))


def test_pair_small_named_masks(dev):
    """The 14 named masks tests/test_mask_cases_cpu.py holds to the oracle's double loop (3 words: one partly filled LDS stage)"""
    m, at = mc.small_masks()
    iou, asy = _pair_case(dev, mc.pack_words(m), "small masks")
    assert iou[at["same_a"], at["same_b"]] == 0x3C00 and iou[at["disj_a"], at["disj_b"]] == 0
    assert asy[at["outer"], at["inner"]] == 0x3C00 and 0 < asy[at["inner"], at["outer"]] < 0x3C00


def test_pair_single_empty_mask(dev):
    iou, asy = _pair_case(dev, np.zeros((2, 1), np.uint64), "one empty mask")
    assert _nan16(iou).all() and _nan16(asy).all()


def test_pair_double_rounding_witness(dev):
    """inter = 683, union = area = 8195: float64 -> float16 directly is one ulp off the reference's float64 -> float32 -> float16
    (recomputed by tests/test_mask_cases_cpu.py), within a tile and across the mirrored tile of one row"""
    w = mc.witness_words()
    iou, asy = _pair_case(dev, w, "witness")
    inter, union = mc.WITNESS
    chain = (np.float64(inter) / np.float64(union)).astype(np.float32).astype(np.float16).view(np.uint16)
    for out in (mc.WIT_OUT_SAME, mc.WIT_OUT_NEXT):
        assert iou[mc.WIT_IN, out] == chain and iou[out, mc.WIT_IN] == chain and asy[mc.WIT_IN, out] == chain
        assert asy[out, mc.WIT_IN] == 0x3C00


# ---- entry-point edges -----------------------------------------------------------------------------------------------------------

def test_n_zero_returns_and_touches_nothing(dev):
    from cim_amd import _lib
    m = _poisoned_u8(torch.zeros(64, dtype=torch.uint8, device=dev))
    words = _OutInt(1, 4, 0, dev, torch.int64)
    _lib.call("cim_mask_pack", m.data_ptr(), words.ptr, 0, 64, _lib.stream_ptr())
    area, iou, asy = _OutInt(1, 4, 0, dev, torch.int32), _OutInt(4, 4, 0, dev, torch.int16), _OutInt(4, 4, 0, dev, torch.int16)
    _lib.call("cim_mask_iou_pair", words.ptr, 0, 1, area.ptr, iou.ptr, asy.ptr, _lib.stream_ptr())
    _lib.call("cim_mask_pack", None, None, 0, 64, _lib.stream_ptr())                 # no pointer is looked at
    _lib.call("cim_mask_iou_pair", None, 0, 1, None, None, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert words.untouched() and area.untouched() and iou.untouched() and asy.untouched()


def test_refusals_launch_nothing(dev):
    from cim_amd import _lib
    m = _poisoned_u8(torch.ones(64, dtype=torch.uint8, device=dev))
    words = _OutInt(1, 1, 0, dev, torch.int64)
    area, iou, asy = _OutInt(1, 1, 0, dev, torch.int32), _OutInt(1, 1, 0, dev, torch.int16), _OutInt(1, 1, 0, dev, torch.int16)
    s = _lib.stream_ptr()
    for args in ((m.data_ptr(), words.ptr, 1, 0),                                    # HW = 0
                 (m.data_ptr(), words.ptr, 1, -64), (m.data_ptr(), words.ptr, -1, 64),
                 (None, words.ptr, 1, 64), (m.data_ptr(), None, 1, 64)):             # a null pointer with N > 0
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_mask_pack", *args, s)
    p = (words.ptr, area.ptr, iou.ptr, asy.ptr)
    for args in ((p[0], 1, 0, p[1], p[2], p[3]),                                     # words = 0
                 (p[0], 1, 1 << 25, p[1], p[2], p[3]),                               # 64 words pixels no longer fit an int
                 (p[0], -1, 1, p[1], p[2], p[3]),
                 (None, 1, 1, p[1], p[2], p[3]), (p[0], 1, 1, None, p[2], p[3]),
                 (p[0], 1, 1, p[1], None, p[3]), (p[0], 1, 1, p[1], p[2], None)):
        with pytest.raises(_lib.CimHipError):
            _lib.call("cim_mask_iou_pair", *args, s)
    torch.cuda.synchronize()
    assert words.untouched() and area.untouched() and iou.untouched() and asy.untouched()


# ---- the wrapper -----------------------------------------------------------------------------------------------------------------

def _forms(h, w):
    """-> [(name, the array to put on the device, the view of it to pass, what that view holds as NumPy [N, H, W])]"""
    n = 70
    u8 = mc.byte_masks(n, h * w, seed=h).reshape(n, h, w)
    i32 = np.array([0, 1, -1, 256, 65536], np.int32)[np.searchsorted(mc.BYTES, u8)]      # 256: zero as a byte, inside as a mask
    f32 = np.array([0.0, 0.5, 1.0, -2.5, 1e-30], np.float32)[np.searchsorted(mc.BYTES, u8)]
    assert (f32 == 0.5).any() and (i32 == 256).any()
    wide = mc.byte_masks(2 * n, h * w, seed=h + 1).reshape(2 * n, h, w)
    turned = np.ascontiguousarray(u8.transpose(0, 2, 1))                                  # [N, W, H] in memory
    same = lambda t: t
    return [("bool", u8 != 0, same, u8 != 0), ("uint8", u8, same, u8), ("int32", i32, same, i32), ("float32", f32, same, f32),
            ("[::2]", wide, lambda t: t[::2], wide[::2]), ("transposed", turned, lambda t: t.transpose(1, 2), u8)]


@pytest.mark.parametrize("h,w", [(9, 13), (12, 11)])                     # HW = 117: the scalar pack kernel; 132: the 16-byte one
def test_wrapper_takes_every_input_form(dev, h, w):
    from cim_amd import mask_iou
    for name, base, view, ref in _forms(h, w):
        d = view(torch.from_numpy(base).to(dev))
        assert tuple(d.shape) == ref.shape and d.is_contiguous() == (name not in ("[::2]", "transposed"))
        words = mc.pack_words(ref != 0)
        assert np.array_equal(mask_iou.pack_masks(d).cpu().numpy().view(np.uint64), words), name
        iou, asy = mask_iou.mask_iou_maps(d)
        riou, rasy, _ = mc.maps_from_words(words)
        assert iou.dtype == torch.float16 and tuple(iou.shape) == (len(ref), len(ref))
        _same_map(iou.cpu().numpy().view(np.uint16), riou, name + " iou")
        _same_map(asy.cpu().numpy().view(np.uint16), rasy, name + " asy")
