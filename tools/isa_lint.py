"""ISA lint of the shipped library: disassemble libenh_hip.so's gfx950 code objects and report, per kernel symbol, the facts DESIGN.md
states about the instruction stream (§3.1c: the tile-claim atomic stays ONE in-flight instruction; §3.1b: the one-wave-per-SIMD kernels
do not touch scratch).  Runs on CPU (llvm-objdump / llvm-readelf of the ROCm toolchain); `tests/test_isa_lint.py` asserts on it.

    python tools/isa_lint.py [path/to/libenh_hip.so]      # prints the table
    python tools/isa_lint.py --diff OLD.so NEW.so         # per kernel symbol: same, or the first differing instruction; exit 1 on any difference
    python tools/isa_lint.py --attention [lib.so]         # the tile loops of the attention kernels: waits, exposed fragment reads, fragment registers
"""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SO = os.path.join(ROOT, "enhancing-transformers_amd", "lib", "libenh_hip.so")


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def code_objects(so_path, workdir):
    """the gfx950 code objects bundled in the .so (llvm-objdump --offloading writes them next to its input: work on a copy)"""
    local = os.path.join(workdir, "lib.so")
    shutil.copy(so_path, local)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], check=True, capture_output=True)
    return sorted(os.path.join(workdir, f) for f in os.listdir(workdir) if "hipv4-amdgcn-amd-amdhsa--gfx950" in f)


def kernel_stats(so_path=DEFAULT_SO):
    """{demangled kernel name: {mbcnt, bcnt1, vmcnt0, atomics, scratch_ops, scratch_bytes, vgpr, agpr, spills, lds}}"""
    stats = collections.defaultdict(lambda: collections.Counter())
    with tempfile.TemporaryDirectory() as wd:
        objs = code_objects(so_path, wd)
        assert objs, f"no gfx950 code object in {so_path}"
        for o in objs:
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", o], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    cur = m.group(1)
                    stats[cur]["_seen"] += 1
                    continue
                if cur is None:
                    continue
                if "v_mbcnt" in line:
                    stats[cur]["mbcnt"] += 1
                if "s_bcnt1" in line:
                    stats[cur]["bcnt1"] += 1
                if "s_waitcnt vmcnt(0)" in line:
                    stats[cur]["vmcnt0"] += 1
                if "global_atomic" in line or "buffer_atomic" in line or "flat_atomic" in line:
                    stats[cur]["atomics"] += 1
                if "scratch_" in line:
                    stats[cur]["scratch_ops"] += 1
                if "v_mfma" in line:
                    stats[cur]["mfma"] += 1
                if "v_max3_f32" in line:
                    stats[cur]["max3"] += 1
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
            for b in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                b = ".agpr_count:" + b
                m = re.search(r"\n\s*\.name:\s*(\S+)\n\s*\.private_segment_fixed_size:\s*(\d+)", b)
                if not m:
                    continue
                k = stats[m.group(1)]
                k["scratch_bytes"] = int(m.group(2))
                for key, pat in (("agpr", r"^\.agpr_count:\s*(\d+)"), ("vgpr", r"\.vgpr_count:\s*(\d+)"), ("spills", r"\.vgpr_spill_count:\s*(\d+)"),
                                 ("lds", r"\.group_segment_fixed_size:\s*(\d+)"), ("sgpr", r"\.sgpr_count:\s*(\d+)")):
                    mm = re.search(pat, b, re.M)
                    if mm:
                        k[key] = int(mm.group(1))
    names = [n for n in stats if "scratch_bytes" in stats[n]]      # kernels only (device functions have no metadata entry)
    dm = _demangle(names)
    return {dm[n]: dict(stats[n]) for n in names}


def kernel_instructions(so_path=DEFAULT_SO):
    """{mangled symbol: [instruction text]} of every function in the .so's gfx950 code objects: mnemonic and operands only (no addresses, encodings,
    comments or directives).  Branches print as offsets relative to themselves; the one operand that does depend on where a function's neighbours lie,
    the literal of the s_add_u32 / s_addc_u32 pair that turns an s_getpc_b64 into the address of a global, is replaced by <pcrel>."""
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        objs = code_objects(so_path, wd)
        assert objs, f"no gfx950 code object in {so_path}"
        for o in objs:
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", o], capture_output=True, text=True, check=True).stdout
            cur, after_getpc = None, 0
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                    continue
                if cur is None or not line.startswith("\t"):
                    continue
                ins = " ".join(line.split("//")[0].split())
                if after_getpc and re.match(r"s_addc?_u32 ", ins):
                    ins = re.sub(r", (0x[0-9a-f]+|\d+)$", ", <pcrel>", ins)
                after_getpc = 2 if ins.startswith("s_getpc_b64") else max(after_getpc - 1, 0)
                cur.append(ins)
    return out


def kernel_listings(so_path=DEFAULT_SO, match="attn_"):
    """{demangled kernel name: [(address, instruction text, branch target address | None)]} for the functions whose mangled name contains `match`"""
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        for o in code_objects(so_path, wd):
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", o], capture_output=True, text=True, check=True).stdout
            cur, start = None, 0
            for line in dis.splitlines():
                m = re.match(r"^([0-9a-f]+) <(.+)>:", line)
                if m:
                    start = int(m.group(1), 16)
                    cur = out.setdefault(m.group(2), []) if match in m.group(2) else None
                    continue
                if cur is None or not line.startswith("\t") or "//" not in line:
                    continue
                text, rest = line.split("//", 1)
                ins = " ".join(text.split())
                addr = int(rest.split(":")[0], 16)
                tgt = None
                if ins.startswith(("s_cbranch", "s_branch")):
                    mm = re.search(r"<.+\+0x([0-9a-f]+)>\s*$", rest)
                    tgt = start + int(mm.group(1), 16) if mm else start
                cur.append((addr, ins, tgt))
    dm = _demangle(list(out))
    return {dm[n]: v for n, v in out.items()}


def _vregs(operand_text):
    regs = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", operand_text):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(a) for a in re.findall(r"\bv(\d+)\b", operand_text))
    return regs


def attention_pipeline(listing):
    """Facts about the TILE LOOP of one attention kernel (a listing of kernel_listings): the span from the lowest target of a backward branch to the
    last backward branch.
      mfma            MFMAs in the loop
      vm_waits        indices (into the loop) of the s_waitcnt that name vmcnt
      closing_ok      True if behind the LAST of them, in layout order and on through the back edge, an s_barrier comes before any MFMA
      exposed         MFMAs whose operand read was issued after the previous MFMA and awaited at once: between the previous MFMA (or the loop's
                      start) and this one there is a ds_read* and, behind it, an s_waitcnt with lgkmcnt(0)
      touched         (index, instruction) of every instruction that names a register an LDS read has been asked to write while that read may still
                      be in flight (LDS operations complete in order; s_waitcnt lgkmcnt(n) leaves the last n in flight).  The asm-issued fragment
                      reads of attention_common.h are invisible to the compiler's own bookkeeping: this is the check that it did not copy, reuse
                      or read such a register between request and wait.
      carried         LDS reads still in flight at a branch or branch target inside the loop (the scan is linear: these are not followed)
      scalar_loads    s_load* / s_buffer_load* in the loop (they share lgkmcnt and complete out of order: the counted waits assume there are none)"""
    back = [(a, t) for a, ins, t in listing if t is not None and t <= a]
    assert back, "no loop"
    lo, hi = min(t for _, t in back), max(a for a, _ in back)
    loop = [(a, ins, t) for a, ins, t in listing if lo <= a <= hi]
    targets = {t for _, _, t in listing if t is not None}
    res = {"mfma": 0, "vm_waits": [], "closing_ok": False, "exposed": 0, "touched": [], "carried": 0, "scalar_loads": 0}
    since_read, since_wait0 = False, False      # since the previous MFMA: a ds_read seen; behind it an lgkmcnt(0) wait seen
    fifo = []                                    # destination registers of the LDS operations in flight, oldest first (empty set: a write)
    for i, (a, ins, t) in enumerate(loop):
        op = ins.split()[0]
        if a in targets or t is not None:
            res["carried"] += sum(1 for d in fifo if d)
            fifo = []
        if op.startswith(("s_load", "s_buffer_load")):
            res["scalar_loads"] += 1
        if op == "s_waitcnt":
            if "vmcnt" in ins:
                res["vm_waits"].append(i)
            m = re.search(r"lgkmcnt\((\d+)\)", ins)
            if m:
                n = int(m.group(1))
                fifo = fifo[len(fifo) - n:] if n else []
                if n == 0 and since_read:
                    since_wait0 = True
            continue
        operands = ins[len(op):]
        used = _vregs(operands)
        for d in fifo:
            if d & used:
                res["touched"].append((i, ins))
                break
        if op.startswith("ds_"):
            fifo.append(_vregs(operands.split(",")[0]) if op.startswith("ds_read") else set())
            if op.startswith("ds_read"):
                since_read, since_wait0 = True, False
        if op.startswith("v_mfma"):
            res["mfma"] += 1
            res["exposed"] += since_wait0
            since_read, since_wait0 = False, False
    if res["vm_waits"]:
        w = res["vm_waits"][-1]
        for a, ins, t in loop[w + 1:] + loop[:w]:      # (the loop's last instruction branches to its first)
            if ins.startswith("s_barrier"):
                res["closing_ok"] = True
            if ins.startswith(("s_barrier", "v_mfma")):
                break
    return res


def diff_instructions(old, new):
    """compare two {symbol: [instruction text]} dictionaries: {symbol: "same" | "only in old" | "only in new" | (index, old instruction, new instruction)}
    with the first difference (None for the side that has ended)"""
    res = {}
    for sym in sorted(set(old) | set(new)):
        if sym not in new or sym not in old:
            res[sym] = "only in old" if sym in old else "only in new"
            continue
        a, b = old[sym], new[sym]
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        res[sym] = "same" if i is None else (i, a[i] if i < len(a) else None, b[i] if i < len(b) else None)
    return res


def diff_main(old_so, new_so):
    res = diff_instructions(kernel_instructions(old_so), kernel_instructions(new_so))
    dm = _demangle(list(res))
    for sym, r in res.items():
        print(f"{dm[sym]}: " + (r if isinstance(r, str) else f"DIFFERS at instruction {r[0]}: {r[1]!r} -> {r[2]!r}"))
    n_same = sum(r == "same" for r in res.values())
    n_one = sum(isinstance(r, str) and r != "same" for r in res.values())
    print(f"isa diff: {n_same} of {len(res)} symbols same, {len(res) - n_same - n_one} differ, {n_one} on one side only")
    return 0 if n_same == len(res) else 1


def persistent_gemm_pairs(stats):
    """(dynamic-schedule symbol, its static-schedule twin) for every persistent GEMM instantiation"""
    pairs = []
    for n in stats:
        m = re.match(r"void (gemm_w256[pr]_kernel)<(.*), true>\(GemmArgs\)$", n)
        if m:
            twin = f"void {m.group(1)}<{m.group(2)}, false>(GemmArgs)"
            assert twin in stats, twin
            pairs.append((n, twin))
    return sorted(pairs)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        if len(sys.argv) != 4:
            sys.exit("usage: isa_lint.py --diff OLD.so NEW.so")
        return diff_main(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 1 and sys.argv[1] == "--attention":
        for name, listing in sorted(kernel_listings(sys.argv[2] if len(sys.argv) > 2 else DEFAULT_SO).items()):
            if "_kernel" in name:
                r = attention_pipeline(listing)
                print(f"{name.split('(')[0]:60s} mfma {r['mfma']:3d} exposed {r['exposed']:3d} vmcnt waits {len(r['vm_waits'])} closing_ok {r['closing_ok']} "
                      f"touched {len(r['touched'])} carried {r['carried']} scalar loads {r['scalar_loads']}")
        return 0
    so = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SO
    st = kernel_stats(so)
    print(f"{len(st)} kernels in {so}")
    print(f"{'kernel':84s} vgpr agpr scratch spills vmcnt0 mbcnt bcnt1 atomics")
    for n in sorted(st):
        s = st[n]
        if s.get("agpr", 0) or s.get("scratch_bytes", 0) or "gemm_w256" in n:
            print(f"{n[:84]:84s} {s.get('vgpr', 0):4d} {s.get('agpr', 0):4d} {s.get('scratch_bytes', 0):7d} {s.get('spills', 0):6d} "
                  f"{s.get('vmcnt0', 0):6d} {s.get('mbcnt', 0):5d} {s.get('bcnt1', 0):5d} {s.get('atomics', 0):7d}")
    bad = 0
    for dyn, sta in persistent_gemm_pairs(st):
        d, s = st[dyn], st[sta]
        ok = d.get("mbcnt", 0) == 0 and d.get("bcnt1", 0) == 0 and d.get("vmcnt0", 0) == s.get("vmcnt0", 0) + 1
        bad += not ok
        if not ok:
            print("LINT", dyn, d, "static twin vmcnt0", s.get("vmcnt0", 0))
    print("persistent-GEMM tile-claim lint:", "FAIL" if bad else "ok", f"({bad} bad)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
