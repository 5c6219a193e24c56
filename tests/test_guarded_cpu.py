"""The guard-band helper itself (tests/guarded.py), on the CPU: a one-byte stray write at every edge is reported with
the buffer's name and side, a full in-bounds write passes, `align` gives exactly that alignment, an input change is reported."""
import numpy as np
import pytest
import torch

import guarded as G


def _arena(fill):
    a = G.Arena("cpu", fill)
    a.request("obs", (5, 49), torch.uint8, 1, init=torch.arange(5 * 49, dtype=torch.int64).to(torch.uint8).view(5, 49))
    a.request("q", (5, 19), torch.float32, 4)
    a.request("frame", (3, 2), torch.int64, 8)
    a.request("cls", (7,), torch.uint8, 1)
    a.request("patch", (3, 32), torch.int32, 16)
    return a


@pytest.mark.parametrize("fill", G.FILLS)
def test_layout(fill):
    a = _arena(fill)
    raw = a.raw()
    assert raw.dtype == torch.uint8 and raw.numel() % 256 == 0 and raw.data_ptr() % 256 == 0
    prev_end = 0
    for name, nbytes in (("obs", 245), ("q", 380), ("frame", 48), ("cls", 7), ("patch", 384)):
        lo, s, e, hi = a.span(name)
        assert e - s == nbytes
        assert lo == prev_end and s - lo >= G.GUARD and hi - e >= G.GUARD   # guards touch the payload and each other
        assert a.take(name).data_ptr() == raw.data_ptr() + s
        prev_end = hi
    assert prev_end == raw.numel()
    a.check()
    a.inputs_unchanged()
    # inputs hold their init, outputs 0x77, everything else `fill`
    assert np.array_equal(a.bytes_of("obs"), np.arange(245, dtype=np.uint8))
    for name in ("q", "frame", "cls", "patch"):
        assert (a.bytes_of(name) == G.OUT_FILL).all()
    assert sorted(a.outputs()) == ["cls", "frame", "patch", "q"]
    n_payload = 245 + 380 + 48 + 7 + 384
    assert int((raw == fill).sum()) >= raw.numel() - n_payload


@pytest.mark.parametrize("align", [1, 4, 8, 16])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.int64])
def test_alignment_is_exact(align, dtype):
    if align < torch.empty((), dtype=dtype).element_size():
        with pytest.raises(AssertionError):
            G.Arena("cpu", 0).request("x", (3,), dtype, align)
        return
    a = G.Arena("cpu", 0)
    a.request("pad", (13,), torch.uint8, 1)
    t = a.take("x", (3, 5), dtype, align)
    p = t.data_ptr()
    assert p % align == 0 and p % (2 * align) != 0
    assert t.dtype == dtype and tuple(t.shape) == (3, 5) and t.is_contiguous()


@pytest.mark.parametrize("fill", G.FILLS)
@pytest.mark.parametrize("name", ["obs", "q", "frame", "cls", "patch"])
@pytest.mark.parametrize("where", ["below", "above", "low_far", "high_far"])
def test_one_stray_byte_is_reported(fill, name, where):
    a = _arena(fill)
    lo, s, e, hi = a.span(name)
    pos, side = {"below": (s - 1, "low"), "above": (e, "high"), "low_far": (s - G.GUARD, "low"),
                 "high_far": (e + G.GUARD - 1, "high")}[where]
    a.raw()[pos] = fill ^ 0x01                      # one bit of one byte
    with pytest.raises(AssertionError) as ei:
        a.check()
    msg = str(ei.value)
    assert repr(name) in msg and f"{side} side" in msg and f"payload offset {pos - s} " in msg
    a.raw()[pos] = fill
    a.check()


@pytest.mark.parametrize("fill", G.FILLS)
def test_full_in_bounds_write_passes(fill):
    a = _arena(fill)
    for name in ("q", "frame", "cls", "patch"):
        t = a.take(name)
        t.view(-1).view(torch.uint8).fill_(0xFF - fill)
        t.zero_()
    a.check()
    a.inputs_unchanged()
    assert all((v == 0).all() for v in a.outputs().values())


@pytest.mark.parametrize("fill", G.FILLS)
def test_input_change_is_reported(fill):
    a = _arena(fill)
    a.inputs_unchanged()
    obs = a.take("obs")
    obs[4, 48] ^= 1
    a.check()                                       # the guards are not involved
    with pytest.raises(AssertionError, match=r"input buffer 'obs' changed: first at byte 244 of 245"):
        a.inputs_unchanged()
    with pytest.raises(AssertionError, match="input buffer 'obs'"):
        a.verify()


@pytest.mark.parametrize("fill", G.FILLS)
def test_inout_buffer(fill):
    """request(..., inout=True): the initial contents are copied in, a change of them is no input change, the whole payload is part of outputs(), and
    its guards are checked like any other's; an in/out buffer without initial contents is refused."""
    ring0 = torch.arange(9 * 5, dtype=torch.int64).to(torch.uint8).view(9, 5)
    a = G.Arena("cpu", fill)
    a.request("obs", (4,), torch.uint8, 1, init=torch.tensor([1, 2, 3, 4], dtype=torch.uint8))
    a.request("ring", (9, 5), torch.uint8, 1, init=ring0, inout=True)
    a.request("q", (3,), torch.float32, 4)
    with pytest.raises(AssertionError, match="starts from its init"):
        a.request("m", (3,), torch.float32, 4, inout=True)
    ring = a.take("ring")
    assert torch.equal(ring, ring0)
    assert sorted(a.outputs()) == ["q", "ring"]
    assert np.array_equal(a.outputs()["ring"], ring0.numpy().reshape(-1))
    ring[3] = 200                                   # the call writes slot 3 ...
    out = a.verify()                                # ... which is no input change
    want = ring0.clone()
    want[3] = 200
    assert np.array_equal(out["ring"].reshape(9, 5), want.numpy())      # every other slot holds its initial contents
    lo, s, e, hi = a.span("ring")
    a.raw()[e] = fill ^ 0x01
    with pytest.raises(AssertionError, match="'ring' changed on its high side"):
        a.verify()
    a.raw()[e] = fill
    a.take("obs")[0] = 9                            # a pure input beside it is still watched
    with pytest.raises(AssertionError, match="input buffer 'obs'"):
        a.verify()


def test_same_bits():
    G.same_bits({"q": np.zeros(4, np.uint8)}, {"q": np.zeros(4, np.uint8)})
    with pytest.raises(AssertionError, match="'q' depends on the guard bytes: first difference at byte 2"):
        G.same_bits({"q": np.zeros(4, np.uint8)}, {"q": np.array([0, 0, 1, 0], np.uint8)})


def test_requests_close_with_the_first_take():
    a = G.Arena("cpu", 0)
    a.take("x", (4,), torch.uint8, 1)
    with pytest.raises(AssertionError):
        a.request("y", (4,), torch.uint8, 1)


def test_wide_guarded_cases_hold_a_done_and_an_auto_reset():
    """The wide environment's guarded cases (tests/test_guarded_gpu.py WIDE: 5 lattices, 6 steps) on the wide C oracle alone: each trajectory
    ends an episode and spends a step on an auto-reset, so the GPU cases exercise both."""
    import test_guarded_gpu as T
    for name in T.WIDE:
        ev = T._wide_oracle_events(name)
        assert ev["done"] >= 1 and ev["reset"] >= 1, (name, ev)
