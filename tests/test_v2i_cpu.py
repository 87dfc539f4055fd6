"""The Python surface of the v2i device-side frame (AnimateChain), checked without a GPU: the Python names import.  (The three entry
points cs_resize_half_bilinear, cs_motion_keypoints_driven and cs_paste_back_shared - declared, typed, bound, exported, the ABI version - are
test_abi_cpu.py's, with every other entry point.)"""


def test_python_names_import():
    from canonswap_amd import tail
    from canonswap_amd.chain import AnimateChain, FrameChain
    from canonswap_amd.engine import Engine
    assert callable(tail.paste_back_shared)
    assert callable(Engine.resize_half_bilinear) and callable(Engine.motion_keypoints_driven)
    for name in ("set_source", "source_state", "load_source_state", "prefetch", "drop_prefetches", "__call__"):
        assert callable(getattr(AnimateChain, name)), name
    assert AnimateChain is not FrameChain
