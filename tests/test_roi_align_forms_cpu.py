"""ROIAlign dispatch (csrc/roi_align.hip): which forward and backward kernel a geometry takes and whether the backward builds the
per-ROI tables, asked of the library on the host (cim_roi_align_forms).  No GPU needed; tests/test_gpu_roi_align_forms.py runs
the same forms on the device against the oracle."""
import importlib
import itertools
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256)


@pytest.fixture(scope="module")
def RA():
    from cim_amd import _lib, build
    build.build()
    _lib.load()
    return importlib.import_module("cim_amd.ops.roi_align")


def test_header_documents_the_forms_and_the_binding_matches(RA):
    from cim_amd import _lib
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define CIM_ROI_((?:FWD|BWD)_[A-Z0-9]+) (\d+)", header)}
    assert values == {n: getattr(RA, n) for n in ("FWD_SAMPLE1", "FWD_SAMPLE4", "FWD_ROWSUM2", "FWD_AGG",
                                                  "BWD_GENERIC1", "BWD_GENERIC4", "BWD_REGION")}
    assert "int cim_roi_align_forms(" in header
    assert _lib.load().cim_roi_align_forms.argtypes == _lib.SIGNATURES["cim_roi_align_forms"]
    assert _lib.load().cim_abi_version() == _lib.ABI_VERSION == 16


def test_backward_reuses_only_tables_the_forward_built(RA):
    """Sweep P 1..17, H and W across every limit, four channel counts, with and without the workspace: the backward that is told
    the tables are ready (what autograd passes after a forward with the workspace) reuses them only where the forward at that
    geometry is a table form.  The geometries where the region backward meets a forward that builds no tables are exactly
    the ones the parent commit read unbuilt tables at; they are listed by rule below."""
    T = (RA.FWD_ROWSUM2, RA.FWD_AGG)
    rebuilt = set()
    for P, H, W, C, ws, K, maskcat in itertools.product(range(1, 18), SIZES, SIZES, (3, 4, 8, 512), (False, True), (1, 1000),
                                                        (False, True)):
        fwd, bwd, builds = RA.forms(1, C, H, W, K, P, maskcat, ws, ws)
        tables = fwd in T
        assert not tables or ws, "a table form without the workspace"
        assert bwd != RA.BWD_REGION or ws, "the region backward without the workspace"
        assert (C % 4 == 0) == (fwd != RA.FWD_SAMPLE1) == (bwd != RA.BWD_GENERIC1)
        if bwd == RA.BWD_REGION and not builds:
            assert tables, "the backward reuses tables the forward never built: %r" % ((P, H, W, C, K, maskcat),)
        assert builds == (bwd == RA.BWD_REGION and not tables)
        assert RA.forms(1, C, H, W, K, P, maskcat, ws, False)[1:] == (bwd, bwd == RA.BWD_REGION)   # tables_ready = 0: always built
        if builds:
            rebuilt.add((P, H, W, C))
    # the geometries (C % 4 == 0, workspace, region backward: maps below 256 x 256 of at most 256 12 x 16 regions) where the
    # forward builds no tables: P 9..16 on any map, P 1..3 on maps of 65..128 rows, any P on maps of 129..255 rows
    assert rebuilt == {(P, H, W, C) for P, H, W, C in itertools.product(range(1, 17), SIZES, SIZES, (4, 8, 512))
                       if H < 256 and W < 256 and ((H + 11) // 12) * ((W + 15) // 16) <= 256
                       and (P > 8 or (H > 64 and (P < 4 or H > 128)))}


@pytest.mark.parametrize("B,C,H,W,K,P,maskcat,fwd,bwd,builds", [
    (1, 1024, 33, 43, 1000, 7, False, "ROWSUM2", "REGION", False),     # the benchmark's backward after the fused forward
    (1, 1024, 33, 43, 1000, 7, True, "ROWSUM2", "REGION", False),
    (2, 64, 112, 150, 40, 7, False, "AGG", "REGION", False),           # VGG16 at scale 1200, landscape
    (2, 64, 150, 112, 40, 7, False, "SAMPLE4", "REGION", True),        # ... portrait
    (1, 64, 33, 43, 40, 14, True, "SAMPLE4", "REGION", True),          # the config default ROI_XFORM_RESOLUTION
    (1, 64, 33, 43, 40, 16, False, "SAMPLE4", "REGION", True),
    (1, 64, 33, 43, 40, 17, False, "SAMPLE4", "GENERIC4", False),
    (1, 32, 64, 40, 40, 8, False, "AGG", "REGION", False),
    (1, 32, 128, 40, 40, 8, False, "AGG", "REGION", False),
    (1, 8, 128, 40, 24, 8, False, "AGG", "REGION", False),             # the tall strip
    (2, 16, 40, 50, 96, 1, False, "ROWSUM2", "REGION", False),
    (2, 16, 40, 50, 96, 3, False, "ROWSUM2", "REGION", False),
    (2, 16, 100, 50, 96, 1, False, "SAMPLE4", "REGION", True),
    (2, 16, 100, 50, 96, 3, False, "SAMPLE4", "REGION", True),
    (1, 16, 128, 129, 40, 4, False, "AGG", "REGION", False),
    (1, 8, 64, 40, 96, 7, False, "ROWSUM2", "REGION", False),
    (1, 8, 65, 40, 96, 7, False, "ROWSUM2", "REGION", False),
    (1, 8, 128, 40, 96, 7, False, "ROWSUM2", "REGION", False),
    (1, 8, 129, 40, 96, 7, False, "SAMPLE4", "REGION", True),
    (1, 8, 255, 40, 96, 7, False, "SAMPLE4", "REGION", True),
    (1, 8, 256, 40, 96, 7, False, "SAMPLE4", "GENERIC4", False),
    (1, 8, 255, 255, 40, 7, False, "SAMPLE4", "GENERIC4", False),      # 22 x 16 regions
    (1, 3, 33, 43, 40, 7, False, "SAMPLE1", "GENERIC1", False),
    (1, 6, 33, 43, 40, 7, True, "SAMPLE1", "GENERIC1", False),
    (1, 516, 33, 43, 40, 7, False, "ROWSUM2", "REGION", False),
    (1, 64, 33, 43, 0, 7, False, "ROWSUM2", "GENERIC4", False),         # no ROIs: the backward only clears grad_in
])
def test_forms_at_named_shapes(RA, B, C, H, W, K, P, maskcat, fwd, bwd, builds):
    assert RA.forms(B, C, H, W, K, P, maskcat) == (getattr(RA, "FWD_" + fwd), getattr(RA, "BWD_" + bwd), builds)
    # without the workspace (CIM_ROI_FWD_EXACT=1, cim_roi_align_fwd / _bwd): sample order and the generic backward
    assert RA.forms(B, C, H, W, K, P, maskcat, False, False) == (
        RA.FWD_SAMPLE4 if C % 4 == 0 else RA.FWD_SAMPLE1, RA.BWD_GENERIC4 if C % 4 == 0 else RA.BWD_GENERIC1, False)


def test_region_backward_limits_follow_lds_and_offsets(RA):
    # P = 16 fits the LDS with 64-ROI groups only: 128-ROI groups (more than 900 workgroups of 64) take the generic backward
    assert RA.forms(1, 512, 37, 49, 1900, 16)[1] == RA.BWD_GENERIC4
    assert RA.forms(1, 512, 37, 49, 1900, 15)[1] == RA.BWD_REGION
    # 32-bit element offsets of the pooled gradient: K P P C (2C for the mask-cat form) < 2^31
    assert RA.forms(1, 2048, 33, 43, 21000, 7, False)[1] == RA.BWD_REGION
    assert RA.forms(1, 2048, 33, 43, 21000, 7, True)[1] == RA.BWD_GENERIC4


def test_forms_rejects_bad_arguments(RA):
    import ctypes
    from cim_amd import _lib
    x = ctypes.c_int()
    for args in ((0, 8, 5, 5, 1, 7), (1, 0, 5, 5, 1, 7), (1, 8, 0, 5, 1, 7), (1, 8, 5, 0, 1, 7), (1, 8, 5, 5, -1, 7),
                 (1, 8, 5, 5, 1, 0), (1, 8, 5, 5, 1, 65536)):
        with pytest.raises(_lib.CimHipError, match="bad argument"):
            RA.forms(*args)
    with pytest.raises(_lib.CimHipError, match="bad argument"):        # tables cannot be ready without a workspace
        RA.forms(1, 8, 5, 5, 1, 7, False, False, True)
    with pytest.raises(_lib.CimHipError, match="bad argument"):
        _lib.call("cim_roi_align_forms", 1, 8, 5, 5, 1, 7, 0, 1, 1, None, ctypes.byref(x), ctypes.byref(x))
