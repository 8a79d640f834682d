"""The visibility-compacted gradient exchange without a GPU: the C ABI declares its entry points,
the trainer has its switches (off by default), and the compact buffer's layout is what the kernels
and the collective's slices assume."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gsr_visibility_pack", "gsr_union_workspace_size", "gsr_union_rows_per_wave", "gsr_union_plan",
         "gsr_rows_gather", "gsr_rows_scatter")


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name


def test_binding_has_the_entry_points():
    from diff_gaussian_rasterization import _C
    for name in NAMES:
        assert hasattr(_C.lib, name), name
    for name in ("visibility_pack", "union_plan", "rows_gather", "rows_scatter", "union_rows_per_wave"):
        assert callable(getattr(_C, name)), name
    rpw = _C.union_rows_per_wave()
    assert rpw > 0 and rpw % 64 == 0
    assert _C.lib.gsr_union_workspace_size(0) == 0 and _C.lib.gsr_union_workspace_size(1000) % 256 == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.visibility_pack(torch.ones(5))


def test_trainer_switches():
    from diff_gaussian_rasterization import multiview
    sig = inspect.signature(multiview.DataParallelTrainer.__init__).parameters
    assert sig["compact_reduce"].default is False and sig["compact_below"].default is None
    g = torch.Generator().manual_seed(1)
    raw = {"xyz": torch.randn(6, 3, generator=g), "f_dc": torch.randn(6, 1, 3, generator=g),
           "f_rest": torch.randn(6, 15, 3, generator=g), "opacity": torch.randn(6, 1, generator=g),
           "scaling": torch.randn(6, 3, generator=g), "rotation": torch.randn(6, 4, generator=g)}
    off = multiview.DataParallelTrainer(raw)
    assert off.compact_reduce is False and off.last_reduce is None and off.reduce() == 0
    on = multiview.DataParallelTrainer(raw, compact_reduce=True)  # constructing it needs no GPU
    assert on.compact_reduce is True and on.compact_below == multiview.COMPACT_BELOW
    assert 0.0 < multiview.COMPACT_BELOW <= 1.0 and round(multiview.COMPACT_BELOW / 0.05, 6).is_integer()
    assert multiview.DataParallelTrainer(raw, compact_reduce=True, compact_below=0.4).compact_below == 0.4
    assert on.reduce() == 0  # no process group: nothing to exchange


def test_compact_layout():
    from diff_gaussian_rasterization.multiview import compact_layout
    # [group][union row][column]: group k starts at U * sum(M_j, j < k); the last entry is the total
    assert compact_layout(10, (3, 3, 45, 1, 3, 4, 1)) == [0, 30, 60, 510, 520, 550, 590, 600]
    assert compact_layout(7, (3, 3, 0, 1, 3, 4, 1)) == [0, 21, 42, 42, 49, 70, 98, 105]
    assert compact_layout(0, (3, 1)) == [0, 0, 0]
    assert compact_layout(1, ()) == [0]
    assert compact_layout(1204, (3, 3, 45, 1, 3, 4, 1))[-1] == 1204 * 60
