"""The face mask from the parser's logits (cs_face_masks; tail.face_masks; the chains' logits=) without a GPU: the C ABI of the entry
point, the Python names, and the yardstick of test_gpu_face_mask.py (tests/face_mask_ref.py) against the reference's fp32 torch lines
(src/can_swap_pipeline_e2e.py:183-190, src/can_swap_pipeline_v2i.py:76-83) on the host."""
import inspect
import os
import re

import pytest
import torch

import face_mask_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_comment_of_the_entry_point_cites_the_reference():
    """(The entry point's types, arity and export: test_abi_cpu.py.)"""
    header = open(os.path.join(ROOT, "include", "canonswap_hip.h")).read()
    comment = re.findall(r"/\*(?:(?!\*/).)*\*/\s*int cs_face_masks", header, flags=re.S)      # the comment right above the declaration
    assert comment and "can_swap_pipeline_e2e.py:183-190" in comment[0] and "can_swap_pipeline_v2i.py:76-83" in comment[0]


def test_python_names_import():
    from canonswap_amd import tail
    from canonswap_amd.can_swap_e2e import can_swapper
    from canonswap_amd.chain import AnimateChain, FrameChain
    assert tail.FACE_VALID == (1, 2, 4, 5, 6, 7, 10, 11, 12) == FR.FACE_VALID
    assert callable(tail.face_masks) and callable(can_swapper.face_masks)
    sig = inspect.signature(tail.face_masks).parameters
    assert list(sig)[:3] == ["e", "logits", "valid"] and sig["valid"].default == tail.FACE_VALID and sig["size"].default == (512, 512)
    assert {"out", "want_labels", "out_labels"} <= set(sig)
    for f in (FrameChain.__call__, FrameChain.prefetch, AnimateChain.set_source):
        assert inspect.signature(f).parameters["logits"].default is None, f
    for cls in (FrameChain, AnimateChain):
        assert inspect.signature(cls.__init__).parameters["valid"].default == tail.FACE_VALID
    assert list(inspect.signature(FrameChain.__call__).parameters)[1:5] == ["crops_u8", "masks", "M_c2o", "frames_ori"]      # positional masks as before
    assert list(inspect.signature(AnimateChain.set_source).parameters)[1:6] == ["crop_u8", "mask", "M_c2o", "img_ori", "driving_id"]


def test_valid_set_word():
    from canonswap_amd import tail
    assert tail.valid_bits(tail.FACE_VALID) == 0x1cf6
    assert tail.valid_bits(()) == 0 and tail.valid_bits(range(32)) == 0xffffffff
    for bad in ((32,), (-1,), (1, 2.5)):
        with pytest.raises(ValueError):
            tail.valid_bits(bad)


@pytest.mark.parametrize("name", sorted(FR.CASES))
def test_yardstick_agrees_with_the_fp32_lines_and_the_inputs_stay_under_the_cap(name):
    """The fp32 torch lines on the host against the float64 yardstick under the tests' own rule, for every input the GPU tests use."""
    ref = FR.reference(name)
    frac = FR.undecided_fraction(ref)
    print(f"{name}: {FR.CASES[name]}: undecided {frac:.3g} of the pixels, smallest margin {float(ref['margin'].min()):.3g}")
    labels, mask = FR.torch_lines(FR.logits_of(name), FR.CASES[name][1])
    FR.assert_agrees(ref, labels, mask, name)
    assert ref["labels"].dtype == torch.uint8 and int(ref["labels"].max()) < FR.CASES[name][0][1]


def test_the_rule_catches_a_wrong_label():
    ref = FR.reference("borders")
    wrong = ref["labels"].clone()
    i = tuple(ref["decided"].nonzero()[0].tolist())
    wrong[i] = (wrong[i] + 1) % 19
    with pytest.raises(AssertionError):
        FR.assert_agrees(ref, wrong, None, "borders")
