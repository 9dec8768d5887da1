"""The register / scratch budget of the evaluation launch's kernel, from the compiler's own remarks (no GPU needed: hipcc
cross-compiles gfx950). `eval_cells_kernel` takes the whole register file by design (one wave per SIMD); what it must not grow
back is scratch: up to round 6 it carried 152 B per lane -- not spills but two 3x3 matrices indexed at run time --, which was half
of the launch's HBM traffic (profiles/r06_eval_scratch_ab.txt)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import helpers  # noqa: E402


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_evaluation_kernel_scratch_budget():
    res = helpers.kernel_resources("eval_kernels.hip")
    cells = [v for k, v in res.items() if "eval_cells_kernel" in k]
    assert len(cells) == 1, sorted(res)
    c = cells[0]
    assert c["ScratchSize"] <= 64, c          # (28 B today: a handful of spilled registers, no private arrays)
    assert c["VGPRs Spill"] <= 32, c
    assert c["Occupancy"] >= 1 and c["VGPRs"] <= 256 and c["AGPRs"] <= 256, c
    # the launches of the route without cell workgroups: no scratch at all
    for k, v in res.items():
        if "eval_jacobian_kernel" in k:
            assert v["ScratchSize"] == 0, (k, v)


def _llvm_tool(name):
    for d in (os.path.join(os.path.dirname(os.path.realpath(entry.HIPCC)), "..", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
@pytest.mark.skipif(not all(_llvm_tool(t) for t in ("clang-offload-bundler", "llvm-readelf", "llvm-objdump", "llvm-objcopy")),
                    reason="no LLVM binary tools")
def test_level_kernels_code_prefetch_stays_in_the_code_object(tmp_path):
    """The barrier form of bcr_level_kernel asks for its own code as data at its first instructions (prefetch_code): it reads
    kLevelCodePrefetchBytes from s_getpc on. Those reads must stay inside the code object's executable segment, which
    depends on where the kernels land in .text: every instantiation without the rolling form is checked."""
    src = os.path.join(entry.CSRC, "bcr_kernels.hip")
    text = open(src).read()
    m = re.search(r"constexpr int kLevelCodePrefetchBytes = ([0-9 *]+);", text)
    assert m, "kLevelCodePrefetchBytes not found"
    nbytes = 1
    for f in m.group(1).split("*"):
        nbytes *= int(f)
    assert "prefetch_code(threadIdx.x, kLevelThreads, kLevelCodePrefetchBytes)" in text
    # the build's object when it is up to date, a fresh compile with the build's flags otherwise
    obj = os.path.join(entry.CSRC, "build", "bcr_kernels.hip.o")
    deps = [src] + [os.path.join(entry.CSRC, f) for f in os.listdir(entry.CSRC) if f.endswith((".hpp", ".h"))]
    if not entry._newer(obj, deps):
        obj = str(tmp_path / "bcr_kernels.o")
        subprocess.run([entry.HIPCC] + entry.HIP_FLAGS + entry.HIP_FILE_FLAGS.get("bcr_kernels.hip", []) + ["-c", src, "-o", obj],
                       check=True, capture_output=True, timeout=900)
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "bcr.co")
    subprocess.run([_llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, str(tmp_path / "host.o")],
                   check=True, capture_output=True)
    subprocess.run([_llvm_tool("clang-offload-bundler"), "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--output=" + co, "--unbundle"], check=True, capture_output=True)
    elf = subprocess.run([_llvm_tool("llvm-readelf"), "--wide", "--segments", "--symbols", co], check=True, capture_output=True,
                         text=True).stdout
    seg_end = None
    for line in elf.splitlines():
        f = line.split()
        if f[:1] == ["LOAD"] and "E" in f[6:-1]:
            seg_end = int(f[2], 16) + int(f[5], 16)      # VirtAddr + MemSiz
    assert seg_end is not None, elf[:2000]
    kernels = {}
    for line in elf.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            k = re.search(r"bcr_level_kernelILb([01])ELb([01])ELb([01])E", f[7])
            if k:
                kernels[k.groups()] = (int(f[1], 16), int(f[2]))
    barrier = {args: v for args, v in kernels.items() if args[2] == "0"}
    assert len(barrier) == 4 and len(kernels) == 5, sorted(kernels)
    for args, (addr, size) in barrier.items():
        dis = subprocess.run([_llvm_tool("llvm-objdump"), "-d", "--start-address=%#x" % addr, "--stop-address=%#x" % (addr + 1024), co],
                             check=True, capture_output=True, text=True).stdout
        g = re.search(r"s_getpc_b64 .*// ([0-9A-Fa-f]+):", dis)
        assert g, ("no s_getpc_b64 at the head of", args)
        pc = int(g.group(1), 16) + 4         # (s_getpc_b64 returns the address of the next instruction)
        assert pc + nbytes <= seg_end, (args, hex(addr), hex(pc), hex(seg_end))
