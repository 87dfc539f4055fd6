"""The one call path into the C ABI, without a GPU and without a built library: canonswap_amd/_lib.py call() and Engine._call against a fake
library that records what it receives.  Everything call() refuses, it refuses before the library is touched."""
import ctypes as C
import glob
import os
import re

import pytest
import torch

from canonswap_amd import _lib
from canonswap_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeLib:
    """Stands where load() keeps the library.  An entry point named in `returns` records its arguments and returns that value; reaching for
    anything else fails the test."""

    def __init__(self, returns, last_error=b"the last error"):
        self.returns, self.last_error, self.calls = returns, last_error, []

    def __getattr__(self, name):
        if name == "cs_last_error":
            return lambda: self.last_error
        if name not in self.returns:
            pytest.fail(f"the library was asked for {name}")
        return lambda *args: self.calls.append((name, args)) or self.returns[name]


@pytest.fixture
def fake(monkeypatch):
    def put(**returns):
        lib = FakeLib(returns)
        monkeypatch.setattr(_lib, "_lib", lib)
        return lib
    return put


class StubStream:
    """Stands for a torch stream: a name, the pointer the library gets, and a record of every wait_stream in `log`, the list the fake library
    records its calls in, so that the order of the two can be read off."""

    def __init__(self, name, cuda_stream, log=None):
        self.name, self.cuda_stream, self.log = name, cuda_stream, log

    def wait_stream(self, other):
        self.log.append(("wait_stream", (self.name, other.name)))

    def __eq__(self, other):                              # torch hands out a new object per current_stream() call: equal by the stream, as there
        return isinstance(other, StubStream) and other.cuda_stream == self.cuda_stream

    __hash__ = None


class Guard:
    def __init__(self, device):
        pass

    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


@pytest.fixture
def ordered(fake, monkeypatch):
    """-> (run, lib): run(name, stream name) drives Engine._call for entry point `name` with that stream current, on a stub engine that has
    seen nothing yet; lib.calls holds the waits and the library's calls in the order they were made."""
    names = ("cs_motion_extract", "cs_soft_erosion", "cs_soft_erosion_frames", "cs_parser", "cs_pack_u8", "cs_swap_frames_ids")
    lib = fake(**{n: 0 for n in names})
    monkeypatch.setattr(torch.cuda, "device", Guard)

    class Stub:
        h, device, _scratch_last, current = C.c_void_p(0x1000), torch.device("cuda:0"), {}, None

        def _stream(self):
            return StubStream(self.current, {"X": 0x10, "Y": 0x20, "Z": 0x30}[self.current], lib.calls)
    e = Stub()

    def run(name, stream):
        e.current = stream
        Engine._call(e, name, *[None] * (len(_lib._TABLES[name][1]) - 2))      # all but the handle and the stream
        assert lib.calls[-1][0] == name and lib.calls[-1][1][-1] == e._stream().cuda_stream      # the call is the last thing made, on that stream
    return run, lib, e


def _waits(lib):
    return [args for name, args in lib.calls if name == "wait_stream"]


def test_a_group_is_ordered_between_streams_and_only_there(ordered):
    run, lib, e = ordered
    run("cs_motion_extract", "X")
    assert _waits(lib) == []
    run("cs_motion_extract", "Y")                         # the same group on another stream: one wait, enqueued before the library is called
    assert [n for n, _ in lib.calls] == ["cs_motion_extract", "wait_stream", "cs_motion_extract"] and _waits(lib) == [("Y", "X")]
    run("cs_motion_extract", "Y")                         # again on Y: nothing further
    assert _waits(lib) == [("Y", "X")]
    run("cs_motion_extract", "X")                         # back on X
    assert _waits(lib) == [("Y", "X"), ("X", "Y")] and lib.calls[-2][0] == "wait_stream"
    run("cs_soft_erosion", "Z")                           # SE's two entry points are one group
    run("cs_soft_erosion_frames", "X")
    assert _waits(lib) == [("Y", "X"), ("X", "Y"), ("X", "Z")]


def test_two_groups_do_not_order_each_other(ordered):
    run, lib, e = ordered
    run("cs_motion_extract", "X")
    run("cs_parser", "Y")
    run("cs_swap_frames_ids", "Z")
    run("cs_soft_erosion_frames", "Y")
    assert _waits(lib) == []
    assert {g: s.name for g, s in e._scratch_last.items()} == {"M": "X", "P": "Y", "G": "Z", "SE": "Y"}


def test_an_entry_point_without_a_row_never_waits(ordered):
    run, lib, e = ordered
    assert "cs_pack_u8" not in _lib.SCRATCH
    run("cs_motion_extract", "X")
    before = dict(e._scratch_last)
    for stream in ("Y", "X", "Z"):
        run("cs_pack_u8", stream)
    assert _waits(lib) == [] and e._scratch_last == before and list(before) == ["M"]
    run("cs_motion_extract", "X")                         # and M's last stream is still X
    assert _waits(lib) == []


def test_one_stream_waits_nowhere(ordered):
    run, lib, e = ordered
    for name in ("cs_motion_extract", "cs_parser", "cs_soft_erosion", "cs_pack_u8", "cs_swap_frames_ids", "cs_soft_erosion_frames") * 2:
        run(name, "X")
    assert _waits(lib) == [] and len(lib.calls) == 12


def test_the_scratch_table():
    assert set(_lib.SCRATCH) <= _lib.TAKES_STREAM
    assert set(_lib.SCRATCH.values()) == {"M", "SE", "P", "A", "G"}
    stage_a = {"cs_motion_extract": "M", "cs_soft_erosion": "SE", "cs_soft_erosion_frames": "SE", "cs_parser": "P"}      # what stage A reaches
    assert {n: _lib.SCRATCH.get(n) for n in stage_a} == stage_a
    assert all(_lib._TABLES[n][1][0] is C.c_void_p for n in _lib.SCRATCH)      # scratch belongs to an engine: each takes the handle


def test_no_placed_wait_remains():
    files = [f for ext in ("py", "hip", "h", "txt") for f in glob.glob(os.path.join(ROOT, "canonswap_amd", "**", "*." + ext), recursive=True)]
    assert len(files) > 30
    left = [(os.path.relpath(f, ROOT), n + 1) for f in files for n, line in enumerate(open(f)) if re.search(r"wait_prefetch|_prefetch_ready", line)]
    assert left == []


def test_an_unknown_name_raises(fake):
    lib = fake()
    with pytest.raises(KeyError, match="cs_no_such_entry"):
        _lib.call("cs_no_such_entry", 1, 2)
    assert lib.calls == []


def test_the_argument_count_is_checked_from_both_sides(fake):
    lib = fake(cs_set_latency_mode=0)
    h = C.c_void_p(1)
    for args, given in (((h, 1, 2), 3), ((h,), 1)):
        with pytest.raises(TypeError, match=rf"cs_set_latency_mode takes 2 arguments, {given} given"):
            _lib.call("cs_set_latency_mode", *args)
    assert lib.calls == []
    _lib.call("cs_set_latency_mode", h, 1)
    assert lib.calls == [("cs_set_latency_mode", (h, 1))]


def test_a_host_tensor_is_no_pointer(fake):
    lib = fake(cs_pack_u8=0)
    h, st = C.c_void_p(1), C.c_void_p(2)
    img, out = torch.zeros(1, 3, 4, 4), C.c_void_p(3)
    with pytest.raises(TypeError, match=r"cs_pack_u8: argument 2 .*cpu"):
        _lib.call("cs_pack_u8", h, 1, img, out, 4, 4, st)
    with pytest.raises(TypeError, match=r"cs_pack_u8: argument 3 .*cpu"):
        _lib.call("cs_pack_u8", h, 1, C.c_void_p(4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 4, 4, st, device=torch.device("cuda:0"))
    assert lib.calls == []


def test_a_tensor_is_no_number(fake):
    lib = fake(cs_pack_u8=0, cs_op_occ_finish=0)
    p = C.c_void_p(1)
    with pytest.raises(TypeError, match="cs_pack_u8: argument 1 .*number"):
        _lib.call("cs_pack_u8", p, torch.tensor(1), p, p, 4, 4, p)
    with pytest.raises(TypeError, match="cs_op_occ_finish: argument 2 .*number"):
        _lib.call("cs_op_occ_finish", p, 49, torch.tensor(0.5), p, 1, 2, 3, p)
    assert lib.calls == []


def test_everything_else_arrives_as_given(fake):
    lib = fake(cs_op_occ_finish=0, cs_swap_ids=0, cs_profile_exec_flops=0)
    a, b = C.c_void_p(8), C.c_void_p(16)
    assert _lib.call("cs_op_occ_finish", a, 49, 0.25, None, 1, 2, 3, b) == 0
    slots, fl = (C.c_int * 2)(1, 2), C.c_double()
    ref = C.byref(fl)
    _lib.call("cs_swap_ids", a, slots, 2, b, None, None)
    _lib.call("cs_profile_exec_flops", a, ref)
    (_, got), (_, got2), (_, got3) = lib.calls
    assert got[0] is a and got[1:3] == (49, 0.25) and got[3] is None and got[4:7] == (1, 2, 3) and got[7] is b      # None: ctypes' NULL
    assert got2[0] is a and got2[1] is slots and got2[2] == 2 and got2[3] is b and got2[4:] == (None, None)
    assert got3[1] is ref


def test_a_status_raises_with_the_last_error(fake):
    lib = fake(cs_finalize_weights=-1, cs_upload=-1, cs_abi_version=4)
    h = C.c_void_p(1)
    with pytest.raises(RuntimeError) as ex:
        _lib.call("cs_finalize_weights", h)
    assert str(ex.value) == "cs_finalize_weights failed: the last error"
    with pytest.raises(RuntimeError) as ex:
        _lib.call("cs_upload", h, b"F.w0", C.c_void_p(2), 64, what="cs_upload(F.w0)")
    assert str(ex.value) == "cs_upload(F.w0) failed: the last error"
    assert [name for name, _ in lib.calls] == ["cs_finalize_weights", "cs_upload"]
    assert "cs_abi_version" not in _lib.STATUS and _lib.call("cs_abi_version") == 4      # the one int that is a value


def test_values_are_returned(fake):
    fake(cs_op_chan_stats_partial_floats=12345, cs_destroy=None)
    assert _lib.call("cs_op_chan_stats_partial_floats", 2, 4096, 32) == 12345
    assert _lib.call("cs_destroy", C.c_void_p(1)) is None


def test_engine_call_puts_the_handle_first_and_the_stream_last(fake, monkeypatch):
    lib = fake(cs_pack_u8=0, cs_set_latency_mode=0)
    guarded = []

    class Guard:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            guarded.append(self.device)

        def __exit__(self, *exc):
            guarded.append(None)
    monkeypatch.setattr(torch.cuda, "device", Guard)

    class Stub:
        h, device, stream, _scratch_last = C.c_void_p(0x1000), torch.device("cuda:0"), 0x2000, {}

        def _stream(self):
            return StubStream("main", self.stream)
    e, img, out = Stub(), C.c_void_p(0x3000), C.c_void_p(0x4000)
    assert "cs_pack_u8" in _lib.TAKES_STREAM and "cs_set_latency_mode" not in _lib.TAKES_STREAM
    Engine._call(e, "cs_pack_u8", 1, img, out, 4, 4)
    assert guarded == [e.device, None]
    Engine._call(e, "cs_set_latency_mode", 1)
    assert lib.calls == [("cs_pack_u8", (e.h, 1, img, out, 4, 4, e.stream)), ("cs_set_latency_mode", (e.h, 1))]
    assert guarded == [e.device, None] * 2
    with pytest.raises(TypeError, match="cs_pack_u8: argument 2 "):      # the engine's device is the one a tensor must be on
        Engine._call(e, "cs_pack_u8", 1, torch.zeros(1, 3, 4, 4), out, 4, 4)
    assert len(lib.calls) == 2


def test_no_spelled_call_remains():
    files = [f for f in glob.glob(os.path.join(ROOT, "canonswap_amd", "*.py")) if os.path.basename(f) != "_lib.py"]
    files.append(os.path.join(ROOT, "tests", "hip_ops.py"))
    assert len(files) > 5
    left = [(os.path.relpath(f, ROOT), n + 1) for f in files for n, line in enumerate(open(f)) if re.search(r"lib\.cs_", line)]
    assert left == []
