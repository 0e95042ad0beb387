"""Host-side checks of the optimizer ranges whose update was applied upstream
(fh_grad_slab.applied, ops.LinearUpdate): validated before anything is launched, so no GPU."""
import pytest
import torch

from fedhip import _lib, ops


def test_slab_array_marks_applied_ranges():
    arr, n = ops._slab_array([(64, 8, None, 0), (8, 36, 8192, 2)])
    assert n == 2
    assert (arr[0].off, arr[0].slab, arr[0].splits, arr[0].applied) == (8, 8192, 2, 0)
    assert (arr[1].off, arr[1].len, arr[1].slab, arr[1].splits, arr[1].applied) == (64, 8, None, 0, 1)


def _sgd(ranges, row_len=64):
    arr, n = ops._slab_array(ranges)
    return _lib.call("fh_sgd_step_slabs", 4096, 4096, 4096, row_len, row_len, 1, arr, n, 0.1, 0.9,
                     0.0, 0, None)


def test_applied_ranges_are_validated_like_slab_ranges():
    for r in ([(2, 8, None, 0)],                       # offset not a float4
              [(8, 6, None, 0)],                       # length not a float4 multiple
              [(60, 8, None, 0)],                      # past the row
              [(8, 8, None, 0), (12, 8, None, 0)],     # overlapping
              [(8, 8, 4096, 2), (12, 8, None, 0)]):    # overlapping a slab range
        with pytest.raises(_lib.FedHipError, match="bad slab range"):
            _sgd(r)
    arr, n = ops._slab_array([(8, 8, 4096, 2)])
    arr[0].applied = 1                                 # applied, yet with a slab
    with pytest.raises(_lib.FedHipError, match="bad slab range"):
        _lib.call("fh_sgd_step_slabs", 4096, 4096, 4096, 64, 64, 1, arr, n, 0.1, 0.9, 0.0, 0, None)


def test_row_applied_everywhere_launches_nothing():
    assert _sgd([(0, 32, None, 0), (32, 32, None, 0)]) == 0


def test_dpsgd_step_refuses_applied_ranges():
    arr, n = ops._slab_array([(8, 8, None, 0)])
    with pytest.raises(_lib.FedHipError, match="slab"):  # no per-image splits, no slab
        _lib.call("fh_dpsgd_step_slabs", 4096, 4096, 4096, 4096, 64, 64, 1, arr, n, 4096, None, 32,
                  64, 0.0, 0, None, 0, 0.1, 0.9, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0.1, 1.0, None, None)


def test_linear_update_falls_back_outside_a_slab_scope():
    """Without a GradSlabs scope, or with views that are not float4 ranges of the collected
    rows, the layer does not fuse (struct() is None: the unfused entry point is issued)."""
    rows = {k: torch.zeros(2, 128) for k in ("P", "G", "S1", "S2")}
    u = ops.LinearUpdate(rows["P"], rows["S1"], rows["S2"], "sgd", 0.1, mode=2)
    w, dw, db = rows["P"][:, :64], rows["G"][:, :64], rows["G"][:, 64:96]
    assert u.struct(None, w, dw, db, 64, 32) is None
    s = ops.GradSlabs("cpu")
    with s.collect(rows["G"]) as d:
        got = u.struct(d, w, dw, db, 64, 32)
        assert got is not None and got[1:] == (0, 64)
        assert got[0].pw == w.data_ptr() and got[0].s1b == rows["S1"].data_ptr() + 4 * 64
        assert got[0].s2w is None and got[0].adam == 0 and got[0].mode == 2
        assert u.struct(d, rows["P"][:, 4:68], dw, db, 64, 32) is None     # not dw's parameter
        assert u.struct(d, w, rows["G"][:, 2:66], db, 64, 32) is None      # not a float4 range
        assert ops.LinearUpdate(rows["P"], rows["S1"], rows["S2"], "sgd", 0.1,
                                mode=0).struct(d, w, dw, db, 64, 32) is None
