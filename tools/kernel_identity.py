"""Per-kernel identity of two builds of libgpusort.so: extracts the gfx950 code object of every object file in two
`gpu-sort_amd/csrc/build` directories (clang-offload-bundler), disassembles them (llvm-objdump -d) and compares kernel by
kernel, plus the kernel metadata (LDS bytes, register counts) from the code objects' notes.

    python tools/kernel_identity.py BASE_BUILD_DIR NEW_BUILD_DIR

Prints one summary line and one line per kernel that differs, is missing or is new; exit status 1 if a kernel of the base
build differs or is missing."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def _kernels(build_dir, tmp, tag):
    code, meta = {}, {}
    for o in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
        base = os.path.join(tmp, tag + "_" + os.path.basename(o))
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + base + ".fb", o])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + base + ".fb",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + base + ".co"])
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                       base + ".co"], text=True)
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
            if m:
                cur = m.group(1)
                code[cur] = []
            elif cur and line.strip():
                code[cur].append(re.sub(r"//.*$", "", line).rstrip())
        # "..." is llvm-objdump's elision of a run of zero bytes.  As the LAST line of a function it is the padding between the
        # function's final instruction and the next symbol, which moves with the link order and is not code: only there is it
        # dropped.  A run of zeros anywhere inside a function is kept and compared.
        # The same holds for the run of `s_nop 0` / `s_code_end` behind a function's final s_endpgm: the assembler's fill up to
        # the next symbol or, for the last kernel of the code object, to the end of the text section -- which kernel that is
        # changes when kernels are added behind it.  Only a run that directly follows an s_endpgm at the end of the listing
        # is dropped.
        for k in code:
            while code[k] and code[k][-1].strip() == "...":
                code[k].pop()
            end = len(code[k])
            while end and code[k][end - 1].strip() in ("s_nop 0", "s_code_end", "..."):
                end -= 1
            if end and code[k][end - 1].strip() == "s_endpgm":
                del code[k][end:]
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", base + ".co"], text=True)
        for block in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name:
                meta[name.group(1)] = sorted(re.findall(r"\.(group_segment_fixed_size|vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\d+)", block))
    return code, meta


def main():
    with tempfile.TemporaryDirectory() as tmp:
        a, ma = _kernels(sys.argv[1], tmp, "base")
        b, mb = _kernels(sys.argv[2], tmp, "new")
    same = [k for k in a if k in b and a[k] == b[k] and ma.get(k) == mb.get(k)]
    diff = [k for k in a if k in b and (a[k] != b[k] or ma.get(k) != mb.get(k))]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    print("symbols in base: %d; identical in new (code and metadata): %d; different: %d; missing in new: %d; new: %d"
          % (len(a), len(same), len(diff), len(gone), len(new)))
    for tag, ks in (("DIFF", diff), ("GONE", gone), ("NEW", new)):
        for k in ks:
            print(tag, k)
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main())
