"""The row-operand rule of ops._rows: which tensor a kernel is handed and with which leading dimension.  Pure stride
arithmetic, so it runs on host tensors.  The rule is re-applied by every backward to the tensors its forward saved: the
last two assertions of _check are what makes that the same number."""
import pytest
import torch

import esc_gnn_amd as E

_rows = E.ops._rows


def _check(t, ld_want, in_place):
    r, ld = _rows(t)
    assert ld == ld_want if isinstance(ld_want, int) else ld_want(ld), (tuple(t.shape), t.stride(), ld)
    assert r.shape == t.shape and torch.equal(r, t)
    assert (r.data_ptr() == t.data_ptr()) == in_place, "copied" if in_place else "not copied"
    assert r.stride(1) == 1 or r.size(1) <= 1
    # what a backward would use for the saved tensor: its stride(0), or the helper again - both are the ld of the forward
    assert r.stride(0) == ld
    again, ld_again = _rows(r)
    assert again is r and ld_again == ld
    return r


def test_a_transposed_column_is_one_row_of_ld_4_without_a_copy():
    col = torch.arange(4.0).view(4, 1)
    t = col.t()
    assert tuple(t.shape) == (1, 4) and t.stride() == (1, 1)          # stride(0) of one row is arbitrary: here below the width
    _check(t, 4, in_place=True)


def test_a_column_slice_of_wider_rows_is_taken_in_place():
    wide = torch.arange(24.0).view(3, 8)
    r = _check(wide[:, 2:6], 8, in_place=True)
    assert r.stride() == (8, 1)
    _check(wide[:1, 2:6], 4, in_place=True)                          # one row of it: the width, still no copy


def test_a_non_unit_inner_stride_is_made_contiguous():
    wide = torch.arange(24.0).view(3, 8)
    r = _check(wide[:, ::2], 4, in_place=False)
    assert r.is_contiguous()
    _check(torch.arange(12.0).view(4, 3).t(), 4, in_place=False)       # [3, 4] with strides (1, 3)
    _check(wide[:1, ::2], 4, in_place=False)
    _check(torch.arange(4.0).expand(3, 4), 4, in_place=False)          # unit inner stride, but the rows overlap (stride(0) = 0)


def test_no_rows():
    _check(torch.zeros(0, 4), lambda ld: ld >= 4, in_place=True)
    _check(torch.zeros(4, 0).t(), lambda ld: ld >= 4, in_place=True)     # [0, 4] with strides (1, 1)
    _check(torch.zeros(0, 8)[:, 2:6], lambda ld: ld >= 4, in_place=True)


def test_required_width():
    wide = torch.arange(24.0).view(3, 8)
    assert _rows(wide[:, 2:5], 3)[1] == 8
    assert _rows(torch.arange(3.0).view(3, 1).t(), 3)[1] == 3
    with pytest.raises(ValueError, match=r"expected a \[N, 3\] tensor, got shape \(3, 8\)"):
        _rows(wide, 3)
    with pytest.raises(ValueError, match=r"expected a \[N, 3\] tensor, got shape \(3,\)"):
        _rows(torch.zeros(3), 3)


def test_not_two_dimensional():
    with pytest.raises(ValueError, match=r"expected a 2-D tensor, got shape \(3,\)"):
        _rows(torch.zeros(3))
    with pytest.raises(ValueError, match=r"expected a 2-D tensor, got shape \(2, 3, 4\)"):
        _rows(torch.zeros(2, 3, 4))
