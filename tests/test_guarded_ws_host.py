"""CPU: the checker of tests/test_gpu_workspace_contract.py checks what it says (tests/helpers/guarded_ws.py on CPU tensors)."""
import pytest
import torch

from tests.helpers.guarded_ws import ALIGN, FILL_BYTES, GUARD, SENTINEL, GuardedWorkspace

CPU = torch.device("cpu")


def _whole(ws, k=-1):
    return ws._live[k]


@pytest.mark.parametrize("fill", FILL_BYTES)
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 4097, 100003])
def test_view_is_exact_aligned_and_filled(fill, nbytes):
    ws = GuardedWorkspace(fill)
    v = ws.get(nbytes, CPU)
    assert v.dtype == torch.uint8 and v.numel() == nbytes and v.is_contiguous()
    assert v.data_ptr() % ALIGN == 0
    assert bool((v == fill).all())
    whole, off, nb = _whole(ws)
    assert nb == nbytes and off >= GUARD and whole.numel() - off - nbytes >= GUARD
    assert nbytes == 0 or v.data_ptr() == whole.data_ptr() + off         # (an empty tensor reports no address)
    assert bool((whole[:off] == SENTINEL).all()) and bool((whole[off + nbytes:] == SENTINEL).all())
    assert SENTINEL not in FILL_BYTES
    assert ws.sizes == [nbytes]
    (n, after), = ws.verify()
    assert n == nbytes and torch.equal(after, torch.full((nbytes,), fill, dtype=torch.uint8))


def test_writes_inside_pass():
    ws = GuardedWorkspace(0xFF)
    v = ws.get(1000, CPU)
    v[0] = 1
    v[999] = 2
    v[1:999] = SENTINEL            # the sentinel's value inside the view is no offence
    (n, after), = ws.verify()
    assert n == 1000 and int(after[0]) == 1 and int(after[999]) == 2


@pytest.mark.parametrize("where", ["one before", "one behind", "first guard byte", "last guard byte"])
def test_a_write_outside_fails(where):
    ws = GuardedWorkspace(0x00)
    ws.get(64, CPU)                 # an intact hand-out first: the failure names the second
    ws.get(1000, CPU)
    whole, off, nb = _whole(ws)
    at = {"one before": off - 1, "one behind": off + nb, "first guard byte": 0, "last guard byte": whole.numel() - 1}[where]
    whole[at] = 0
    with pytest.raises(AssertionError, match=rf"hand-out 1 \(1000 bytes\).*offset {at - off} "):
        ws.verify()


def test_each_get_refills_and_nothing_is_shared():
    ws = GuardedWorkspace(0xFF)
    a = ws.get(512, CPU)
    a.zero_()
    b = ws.get(512, CPU)
    assert bool((b == 0xFF).all()) and bool((a == 0).all())
    assert a.data_ptr() != b.data_ptr()
    assert ws.current(CPU).data_ptr() == b.data_ptr()
    got = ws.verify()
    assert [n for n, _ in got] == [512, 512] and bool((got[0][1] == 0).all()) and bool((got[1][1] == 0xFF).all())
    assert ws.current(CPU) is None and ws.sizes == [512, 512]
    assert ws.verify() == []


def test_second_hand_reproduces_its_bytes():
    g = torch.Generator().manual_seed(0)
    first = GuardedWorkspace(0xFF)
    for n in (300, 0, 77):
        v = first.get(n, CPU)
        v.copy_(torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g))
    left = first.verify()
    ws = GuardedWorkspace([t for _, t in left])
    for n, t in left:
        v = ws.get(n, CPU)
        assert torch.equal(v, t) and (n == 0 or v.data_ptr() != t.data_ptr())
        v.zero_()                   # the capture is not the buffer handed out
    assert all(torch.equal(a[1], b) for a, b in zip(left, [t for _, t in left]))
    assert int(left[0][1].sum()) > 0
    ws.verify()


def test_second_hand_size_mismatch_is_an_error():
    ws = GuardedWorkspace([torch.zeros(300, dtype=torch.uint8)])
    with pytest.raises(AssertionError, match="300"):
        ws.get(301, CPU)
    ws = GuardedWorkspace([torch.zeros(300, dtype=torch.uint8)])
    ws.get(300, CPU)
    with pytest.raises(AssertionError, match="holds only 1"):
        ws.get(300, CPU)


def test_only_the_two_fill_bytes():
    with pytest.raises(AssertionError):
        GuardedWorkspace(0xAB)
