"""Engine._call on the device: a tensor the kernels could not read is refused before anything launches, a device tensor arrives as its address."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def e():
    from canonswap_amd.engine import Engine
    eng = Engine(0, max_batch=1)      # cs_pack_u8 needs no weights
    yield eng
    eng.close()


def _img():
    return (torch.arange(48, dtype=torch.float32) / 47).reshape(1, 3, 4, 4)


def _refused(e, img):
    out = torch.full((1, 4, 4, 3), 7, dtype=torch.uint8, device=e.device)
    with pytest.raises(TypeError, match="cs_pack_u8: argument 2 "):
        e._call("cs_pack_u8", 1, img, out, 4, 4)
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def test_a_host_tensor_is_refused_and_nothing_launches(e):
    _refused(e, _img())


def test_a_device_tensor_arrives_as_its_address(e):
    img = _img().to(e.device)
    out = torch.full((1, 4, 4, 3), 7, dtype=torch.uint8, device=e.device)
    e._call("cs_pack_u8", 1, img, out, 4, 4)
    assert torch.equal(out, e.pack_u8(img)) and not bool((out == 7).all())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_a_tensor_on_another_device_is_refused(e):
    _refused(e, _img().to("cuda:1"))
