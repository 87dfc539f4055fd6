"""Disassembly checks of the hand-counted wait rings in the built objects (run by __graft_entry__.build())."""
from __future__ import annotations

import os
import subprocess

from ._build import HALO_NGROUPS, OBJ_DIR


def _disassemble(obj_dir: str, objdump: str, oname: str) -> str:
    """Disassembly of the gfx950 code object inside obj_dir/oname; the files the extraction leaves next to the object are removed again."""
    obj = os.path.join(obj_dir, oname)
    subprocess.run([objdump, "--offloading", obj], check=True, capture_output=True)
    co = obj + ".0.hipv4-amdgcn-amd-amdhsa--gfx950"
    try:
        return subprocess.run([objdump, "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    finally:
        for f in os.listdir(obj_dir):
            if f.startswith(oname + ".0."):
                os.remove(os.path.join(obj_dir, f))


def isa_check(obj_dir: str | None = None) -> dict:
    """Compile-time guard for the hand-counted weight ring of the dynamic-shape conv kernels (conv_halo_kernel.h, ST = 0).

    Those kernels stream weight fragments with inline-asm `global_load_dwordx4` the compiler does not track and wait for them with
    an explicit `s_waitcnt vmcnt(WCH * (PFD - 1))`.  A compiler change that moves, duplicates or drops one of these would read stale
    registers without any diagnostic.  This disassembles every conv_halo object and checks, per
    ST = 0 kernel: exactly PFD = 4 counted waits `s_waitcnt vmcnt(3 * WCH)`; the 4 x WCH fragments of the ring in 16 WCH distinct registers;
    after each wait, for every fragment of the slot, an MFMA whose weight operand is that fragment's registers, and then that slot's reload (WCH `global_load_dwordx4` into the same registers the prologue primed it with); and the
    final `s_waitcnt vmcnt(0)` drain before the epilogue.  Raises RuntimeError on any mismatch; returns {kernel: waits found}."""
    import re
    obj_dir = obj_dir or OBJ_DIR
    objdump = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
    if not os.path.exists(objdump):
        raise FileNotFoundError(f"isa_check: {objdump} not found")      # build() reports the check as skipped; a failed check is a RuntimeError
    seen = dict(_isa_check_wide(obj_dir, objdump))
    seen.update(_isa_check_lat(obj_dir, objdump))
    for g in range(HALO_NGROUPS):
        txt = _disassemble(obj_dir, objdump, f"conv_halo_g{g}.o")
        for m in re.finditer(r"^[0-9a-f]+ <(_Z16conv_halo_kernelILi\d+ELi\d+ELi(\d+)ELi\d+ELi\d+ELi\d+ELb[01]ELb[01]ELi0EEv10ConvParams)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)",
                             txt, re.S | re.M):
            name, wch, body = m.group(1), int(m.group(2)), m.group(3).split("\n")
            want = f"s_waitcnt vmcnt({3 * wch})"
            kend = max(i for i, l in enumerate(body) if "v_mfma" in l)        # the epilogue's own (compiler-counted) waits are not the ring's
            waits = [i for i, l in enumerate(body) if i < kend and l.strip().startswith(want) and "lgkmcnt" not in l]
            if len(waits) < 4:
                raise RuntimeError(f"isa_check: {name}: {len(waits)} x `{want}` in the K loop, expected 4 (one per ring slot)")
            waits = waits[:4]     # (a later wait with the same count is the compiler's own, for the spill stores of the loop's drain)
            loads = [(i, re.search(r"global_load_dwordx4 v\[(\d+):(\d+)\], v\[\d+:\d+\], off", l)) for i, l in enumerate(body)]
            loads = [(i, int(q.group(1))) for i, q in loads if q]
            prime = [r for i, r in loads if i < waits[0]][-4 * wch:]          # the ring as the prologue primed it: 4 slots x WCH fragments
            if len(prime) != 4 * wch:
                raise RuntimeError(f"isa_check: {name}: the prologue primes {len(prime)} ring registers, expected {4 * wch}")
            if len({r + j for r in prime for j in range(4)}) != 16 * wch:      # (what a spilled slot looks like: two fragments in v[52:55] and v[50:53])
                raise RuntimeError(f"isa_check: {name}: the ring's fragments overlap in registers: v{sorted(prime)}")
            for k, w in enumerate(waits):
                slot = prime[k * wch:(k + 1) * wch]
                end = waits[k + 1] if k + 1 < 4 else len(body)
                seg = body[w:end]
                rel = [i for i, r in loads if w < i < end and r in slot]
                if len(rel) < wch:
                    raise RuntimeError(f"isa_check: {name}: ring slot {k} is not reloaded into v{slot} after its wait")
                first_reload = min(rel) - w
                uses = [j for j, l in enumerate(seg[:first_reload]) if "v_mfma" in l and any(f"v[{r}:{r + 3}]" in l for r in slot)]
                if not uses:
                    raise RuntimeError(f"isa_check: {name}: no MFMA reads ring slot {k} (v{slot}) between its wait and its reload")
                # every fragment of the slot, not a copy of it: a copy or a spill made before the untracked load landed holds stale data
                for r in slot:
                    if not any("v_mfma" in l and re.search(rf"v_mfma\S+ [av]\[\d+:\d+\], v\[{r}:{r + 3}\],", l) for l in seg[:first_reload]):
                        raise RuntimeError(f"isa_check: {name}: no MFMA takes v[{r}:{r + 3}] of ring slot {k} as its weight operand (a copy or a spill of the ring?)")
            tail = "\n".join(body[waits[-1]:])
            if "s_waitcnt vmcnt(0)" not in tail:
                raise RuntimeError(f"isa_check: {name}: the ring is not drained (s_waitcnt vmcnt(0)) before the epilogue")
            seen[name] = len(waits)
    if not seen:
        raise RuntimeError("isa_check: no dynamic-shape conv_halo kernel found in the objects (name mangling changed?)")
    return seen


def _isa_check_lat(obj_dir: str, objdump: str) -> dict:
    """conv_lat.hip stages its halo with LDS-DMA instructions hidden from the compiler (inline asm) next to compiler-counted weight loads,
    and waits for a chunk's DMA at the chunk's head with a hand-counted `s_waitcnt vmcnt(N)` + `s_barrier`.  vmcnt retires in order, so the
    wait covers a DMA piece iff at least N vector-memory instructions were issued after it.  Check that for every DMA piece of every such
    kernel at the first barrier-wait behind it, and that 8 chunks x 6 K-steps of MFMAs sit between 10 barriers (straight-line code)."""
    import re
    txt = _disassemble(obj_dir, objdump, "conv_lat.o")
    seen = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\S*conv_lat_kernel\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", txt, re.S | re.M):
        name, body = m.group(1), [l.split("//")[0].strip() for l in m.group(2).split("\n")]
        body = [l for l in body if l]
        mf = [i for i, l in enumerate(body) if l.startswith("v_mfma")]
        if not mf:
            raise RuntimeError(f"isa_check: {name}: no MFMA")
        if any(l.startswith(("s_cbranch", "s_branch")) for l in body[mf[0]:mf[-1]]):
            raise RuntimeError(f"isa_check: {name}: a branch inside the K loop (the walk assumes straight-line code)")
        # m0 belongs to the hidden DMA: `s_mov_b32 m0, sN` is legal only as the head of `s_mov_b32 m0 | s_nop | buffer_load ... lds`, and nothing else
        # in the kernel may read or write it (a compiler that started to keep a value in m0 would be caught here)
        for i, l in enumerate(body):
            if re.search(r"\bm0\b", l):
                ok = l.startswith("s_mov_b32 m0,") and any(b.startswith("buffer_load") and b.endswith("lds") for b in body[i + 1:i + 3])
                if not ok:
                    raise RuntimeError(f"isa_check: {name}: `{l}` touches m0 outside the hidden LDS-DMA sequence")
        nvm, open_dma, nbar, ndma = 0, [], 0, 0
        for i, l in enumerate(body[:mf[-1] + 1]):
            op = l.split()[0]
            if op.startswith(("global_load", "buffer_load", "global_store", "buffer_store", "scratch_load", "scratch_store")):
                if op.startswith("buffer_load") and l.endswith("lds"):
                    open_dma.append(nvm); ndma += 1
                nvm += 1
            if op == "s_barrier":
                nbar += 1
                # the wait that covers this barrier: the nearest vmcnt wait above it
                w = next((body[j] for j in range(i - 1, max(i - 6, -1), -1) if body[j].startswith("s_waitcnt") and "vmcnt" in body[j]), None)
                if w is None and not open_dma:
                    continue          # (the reduction's barriers behind the last chunk: nothing is in flight)
                if w is None:
                    raise RuntimeError(f"isa_check: {name}: barrier {nbar} of the K loop has no vmcnt wait in front of it")
                n = int(re.search(r"vmcnt\((\d+)\)", w).group(1))
                for idx in open_dma:      # every piece issued so far is this chunk's (the next chunk's go out behind the barrier)
                    if nvm - idx - 1 < n:
                        raise RuntimeError(f"isa_check: {name}: `{w}` before barrier {nbar} does not cover a DMA piece issued {nvm - idx - 1} vector-memory instructions earlier")
                open_dma = []
        if open_dma:
            raise RuntimeError(f"isa_check: {name}: {len(open_dma)} DMA pieces are never waited for at a chunk head")
        if len(mf) not in (8 * 6 * 8, 8 * 6 * 16) or ndma != 24:
            raise RuntimeError(f"isa_check: {name}: {len(mf)} MFMAs / {ndma} DMA instructions, expected 384 or 768 / 24")
        seen[name] = len(mf)
    if not seen:
        raise RuntimeError("isa_check: no conv_lat kernel found in conv_lat.o (name mangling changed?)")
    return seen


def _isa_check_wide(obj_dir: str, objdump: str) -> dict:
    """conv_wide.hip and the 256 x 160 tiles of conv_halo (ASMR) stream their weight ring with untracked inline-asm loads and wait with
    counted `s_waitcnt vmcnt(N)` that name the slot's registers.  Check in the disassembly of every such kernel: each MFMA's weight operand
    (src0) is a VGPR quadruple whose last writer is a `global_load_dwordx4` (never a copy of one: a copy made before the data landed would
    be stale) with a vmcnt wait between that load and the MFMA; conv_wide: 18 K-steps x 64 MFMAs per kernel."""
    seen = _isa_check_ring(obj_dir, objdump, "conv_wide.o", r"\S*conv_wide_kernel\S*", 18 * 64)
    seen.update(_isa_check_ring(obj_dir, objdump, "conv_halo_g1.o", r"_Z16conv_halo_kernelILi32ELi8ELi5ELi2ELi2ELi0ELb1ELb0ELi[789]E\S*", None))
    return seen


def _isa_check_ring(obj_dir: str, objdump: str, oname: str, name_re: str, expect_mfma) -> dict:
    import re
    txt = _disassemble(obj_dir, objdump, oname)
    seen = {}
    for m in re.finditer(r"^[0-9a-f]+ <(" + name_re + r")>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", txt, re.S | re.M):
        name, body = m.group(1), m.group(2).split("\n")
        writer, waited, issued, nmfma = {}, {}, {}, 0      # issued[r]: VMEM ops issued before the load that last wrote v<r>
        pending, nvm = [], 0          # ring loads in flight: (destination registers, VMEM ops issued before it); VMEM ops issued so far
        mf = [i for i, l in enumerate(body) if "v_mfma" in l]
        lo, hi = (mf[0], mf[-1]) if mf else (0, 0)      # the in-flight check follows the K loop and what lies behind it up to the drain (straight-line there)
        for li, l in enumerate(body):
            t = l.split("//")[0].strip()
            if not t:
                continue
            op = t.split()[0]
            if op.startswith("s_waitcnt") and "vmcnt" in t:
                n = int(re.search(r"vmcnt\((\d+)\)", t).group(1))
                for r in waited:          # vmcnt(n) leaves at most the n youngest VMEM ops outstanding: a load is covered only if it is older
                    if nvm - issued.get(r, -1) - 1 >= n:
                        waited[r] = True
                pending = [q for q in pending if nvm - q[1] - 1 < n]          # at most n VMEM ops are outstanding: the older ones have landed
            # a load the compiler does not track writes its registers when the data lands, not where the instruction stands: nothing else may
            # write them before a counted wait covers the load (the bug this guards against: a fetch whose result nobody reads looks dead to the
            # register allocator, which hands its destination to another value)
            if op.startswith(("s_cbranch", "s_branch", "s_endpgm")) or li < lo:
                pending = []          # (the walk is textual: across a branch the issue order is not the text order)
            if pending and not op.startswith(("s_", "global_store", "buffer_store", "ds_write", "scratch_store")):
                mm0 = re.match(r"\S+\s+(v\[(\d+):(\d+)\]|v(\d+))", t)
                if mm0 and not (op.startswith("buffer_load") and t.endswith("lds")):
                    dst = set(range(int(mm0.group(2)), int(mm0.group(3)) + 1)) if mm0.group(2) else {int(mm0.group(4))}
                    for regs, _ in pending:
                        if regs & dst:
                            raise RuntimeError(f"isa_check: {name}: `{t}` writes v{sorted(regs & dst)} while an untracked ring load into them is in flight")
            if op.startswith(("global_load", "buffer_load", "global_store", "buffer_store", "scratch_load", "scratch_store", "global_atomic")):
                if op.startswith("global_load_dwordx4") and li >= lo:
                    q = re.match(r"\S+\s+v\[(\d+):(\d+)\]", t)
                    if q:
                        pending.append((set(range(int(q.group(1)), int(q.group(2)) + 1)), nvm))
                nvm += 1
            if op.startswith("v_mfma"):
                ops = re.findall(r"([av])\[(\d+):(\d+)\]", t)
                if len(ops) < 4 or ops[1][0] != "v":
                    raise RuntimeError(f"isa_check: {name}: MFMA with a weight operand outside the VGPRs: {t}")
                nmfma += 1
                for r in range(int(ops[1][1]), int(ops[1][2]) + 1):
                    if not writer.get(r, "").startswith("global_load_dwordx4"):
                        raise RuntimeError(f"isa_check: {name}: v{r}, a weight operand of `{t}`, was last written by `{writer.get(r)}` (a copy of a ring register?)")
                    if not waited.get(r, False):
                        raise RuntimeError(f"isa_check: {name}: no vmcnt wait between the ring load of v{r} and `{t}`")
                continue
            if op.startswith(("global_store", "buffer_store", "ds_write", "scratch_store", "s_", "buffer_load_dwordx4")) and "lds" in t + " lds" and not op.startswith("global_load"):
                if not op.startswith(("v_", "ds_read", "global_load", "scratch_load")):
                    continue
            mm = re.match(r"\S+\s+(v\[(\d+):(\d+)\]|v(\d+))", t)
            if mm and not op.startswith(("global_store", "buffer_store", "ds_write", "scratch_store")) and not (op.startswith("buffer_load") and t.endswith("lds")):
                rng = range(int(mm.group(2)), int(mm.group(3)) + 1) if mm.group(2) else [int(mm.group(4))]
                is_vm = op.startswith(("global_load", "buffer_load", "scratch_load"))
                for r in rng:
                    writer[r] = op
                    waited[r] = False
                    issued[r] = (nvm - 1) if is_vm else -1      # (nvm was advanced for this load above)
        if expect_mfma is not None and nmfma != expect_mfma:
            raise RuntimeError(f"isa_check: {name}: {nmfma} MFMAs in the kernel, expected {expect_mfma}")
        seen[name] = nmfma
    if not seen:
        raise RuntimeError(f"isa_check: no kernel matching {name_re} found in {oname} (name mangling changed?)")
    return seen
