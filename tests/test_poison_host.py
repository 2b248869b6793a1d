"""CPU: the scratch-poison helpers of tests/_poison.py (what tests/test_gpu_scratch.py stands on), with ``devices=("cpu",)``."""
import math

import pytest
import torch

from _poison import poison_, poison_buffers, poisoned_allocations


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16])
def test_poison_reads_as_nan_in_every_float_type(dtype):
    t = poison_(torch.zeros(3, 5, dtype=dtype))
    assert torch.isnan(t).all() and (_bytes(t) == 0xFF).all()


def test_poison_byte_patterns_of_the_integer_types():
    assert (poison_(torch.zeros(7, dtype=torch.int32)) == -1).all()
    assert (poison_(torch.zeros(7, dtype=torch.int64)) == -1).all()
    assert (poison_(torch.zeros(7, dtype=torch.uint8)) == 255).all()
    assert (poison_(torch.zeros(2, 2, dtype=torch.int8)) == -1).all()


def test_poison_of_zero_dim_empty_and_strided_tensors():
    s = poison_(torch.zeros((), dtype=torch.float64))
    assert s.dim() == 0 and math.isnan(s.item())
    e = poison_(torch.zeros(0, 4))
    assert e.shape == (0, 4)
    e = poison_(torch.zeros(0, dtype=torch.uint8))
    assert e.numel() == 0
    # a strided view: its elements and nothing between them
    base = torch.zeros(6, 8)
    v = base[:, :5]
    assert not v.is_contiguous()
    assert poison_(v) is v
    assert torch.isnan(base[:, :5]).all() and (base[:, 5:] == 0).all()
    assert (_bytes(base[:, :5]) == 0xFF).all()
    w = torch.zeros(4, 4, dtype=torch.int32)
    poison_(w.t()[1:3])
    assert (w[:, 1:3] == -1).all() and (w[:, 0] == 0).all() and (w[:, 3] == 0).all()
    # a contiguous slice of a larger buffer: the neighbours stay
    b = torch.zeros(16, dtype=torch.uint8)
    poison_(b[4:12].view(torch.float32))
    assert (b[:4] == 0).all() and (b[4:12] == 255).all() and (b[12:] == 0).all()


def test_poisoned_allocations_fills_counts_and_restores():
    e0, el0 = torch.empty, torch.empty_like
    with poisoned_allocations(devices=("cpu",)) as count:
        assert torch.empty is not e0 and torch.empty_like is not el0
        a = torch.empty(4, 3)
        b = torch.empty((5,), dtype=torch.float64)
        c = torch.empty_like(torch.zeros(2, dtype=torch.int32))
        d = torch.empty(0)
        z = torch.zeros(3)                        # (not an uninitialised allocation: untouched)
        assert count.tensors == 4 and count.bytes == 4 * 3 * 4 + 5 * 8 + 2 * 4
    assert torch.empty is e0 and torch.empty_like is el0
    assert torch.isnan(a).all() and torch.isnan(b).all() and (c == -1).all() and d.numel() == 0 and (z == 0).all()
    assert a.dtype == torch.float32 and a.shape == (4, 3) and b.dtype == torch.float64 and c.dtype == torch.int32
    assert "tensors=4" in repr(count)


def test_poisoned_allocations_leaves_other_devices_alone():
    with poisoned_allocations() as count:         # (the default: device memory only)
        torch.empty(8)
        torch.empty_like(torch.ones(3))
    assert count.tensors == 0 and count.bytes == 0
    with poisoned_allocations(devices=(torch.device("cpu"),)) as count:
        torch.empty(8, device="meta")
        torch.empty(2, device="cpu")
    assert count.tensors == 1 and count.bytes == 8


def test_poisoned_allocations_restores_after_an_exception_and_nests():
    e0, el0 = torch.empty, torch.empty_like
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned_allocations(devices=("cpu",)):
            raise RuntimeError("boom")
    assert torch.empty is e0 and torch.empty_like is el0
    with poisoned_allocations(devices=("cpu",)) as outer:
        with poisoned_allocations(devices=("cpu",)) as inner:
            torch.empty(2)
        torch.empty(3)
    assert torch.empty is e0 and torch.empty_like is el0
    assert inner.tensors == 1 and outer.tensors == 2 and outer.bytes == 20


def test_poison_buffers_walks_nested_tables_and_keeps_what_it_is_told_to():
    class Engine:
        pass
    eng = Engine()
    eng._buf = {
        "A32": torch.zeros(3, 3),
        "Qe32_pad": torch.zeros(2, 4),
        "info": torch.zeros(1, dtype=torch.int32),
        ("dp_bufs", 600, 2): dict(wire=torch.zeros(5), q_local=torch.zeros(2, 2), q_all=torch.zeros(2, 2)),
        "nest": {"inner": {"deep": torch.zeros(2)}, "kept": torch.zeros(2)},
        "pair": (torch.zeros(1), torch.zeros(1)),
        "not_a_tensor": 3,
    }
    dp = repr(("dp_bufs", 600, 2))
    done = poison_buffers(eng, keep={"Qe32_pad", dp + "/wire", dp + "/q_local", "nest/kept"})
    assert done == sorted(["A32", "info", dp + "/q_all", "nest/inner/deep", "pair[0]", "pair[1]"])
    assert torch.isnan(eng._buf["A32"]).all() and (eng._buf["info"] == -1).all()
    assert (eng._buf["Qe32_pad"] == 0).all() and (eng._buf["nest"]["kept"] == 0).all()
    d = eng._buf[("dp_bufs", 600, 2)]
    assert (d["wire"] == 0).all() and (d["q_local"] == 0).all() and torch.isnan(d["q_all"]).all()
    assert torch.isnan(eng._buf["nest"]["inner"]["deep"]).all() and torch.isnan(eng._buf["pair"][1]).all()
    # a plain dict, an outer name that covers its whole nest, an empty keep
    table = {"x": torch.zeros(2), "grp": {"a": torch.zeros(1), "b": torch.zeros(1)}}
    assert poison_buffers(table, keep=("grp",)) == ["x"]
    assert (table["grp"]["a"] == 0).all()
    assert poison_buffers(table) == ["grp/a", "grp/b", "x"]
    assert poison_buffers({}) == []
