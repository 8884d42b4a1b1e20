"""Do two builds of libsrgpt_hip compile to the same machine code?

    python scripts/compare_isa.py OLD_CSRC_DIR NEW_CSRC_DIR

Each argument is a `spatialrgpt_amd/csrc` directory after `make -j16 ARCH=gfx950`.  The gfx950 code object of every `*.o` is
unbundled and its kernels (the `*.kd` symbols) are compared: the new build's kernels must be a subset of the old build's, and every
kernel kept must have the same instructions (`llvm-objdump -d`, addresses and encodings stripped) and the same metadata (SGPR / VGPR /
AGPR counts, spills, LDS, scratch, kernarg size, wavefront size).  Kernels only the old build has are listed as removed.  Prints
"identical" when every kept kernel matches, otherwise the first kernel that differs (exit status 1).

This is the check for a change of `csrc/` that must not change the product's kernels.  A change that does is measured on the GPU
between two builds of the library instead (`ab_libs_decode_step.sh`).
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META_KEYS = (".agpr_count", ".sgpr_count", ".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".kernarg_segment_size", ".wavefront_size", ".max_flat_workgroup_size",
             ".uses_dynamic_stack")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], capture_output=True, text=True, check=True).stdout


def code_object(obj, out):
    """the gfx950 device ELF of a hipcc object: its .hip_fatbin section is an offload bundle"""
    fatbin = out + ".fatbin"
    tool("llvm-objcopy", f"--dump-section=.hip_fatbin={fatbin}", obj, out + ".host")
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fatbin}", f"--output={out}")
    return out


def instructions(elf):
    """{kernel symbol: instruction lines}"""
    dis = tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "--mcpu=gfx950", elf)
    body, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^<(.+)>:$", ln.strip())
        if m:
            cur = body.setdefault(m.group(1), [])
            continue
        ln = ln.split("//")[0].strip()  # the trailing comment holds the address, the encoding and branch targets
        if cur is not None and ln and ln != "...":  # ("...": zero padding up to the next symbol)
            cur.append(ln)
    return body


def metadata(elf):
    """{kernel symbol: sorted metadata lines} from the amdhsa.kernels list of the metadata note"""
    meta, entry, sym = {}, [], None
    for ln in tool("llvm-readelf", "--notes", elf).splitlines() + ["  - end"]:
        if ln.startswith("  - "):  # a new kernel entry (deeper list items are argument descriptors)
            if sym:
                meta[sym] = sorted(entry)
            entry, sym = [], None
        item = ln[4:] if ln.startswith(("  - ", "    ")) and not ln.startswith("     ") else ""
        key = item.split(":")[0]
        if key == ".symbol":
            sym = item.split(":", 1)[1].strip()[: -len(".kd")]
        elif key in META_KEYS:
            entry.append(" ".join(item.split()))
    return meta


def collect(csrc, tmp):
    """{(object file, kernel symbol): (instructions, metadata)}"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(csrc, "*.o"))):
        base = os.path.basename(obj)
        elf = code_object(obj, os.path.join(tmp, base + ".co"))
        names = re.findall(r"\s(\S+)\.kd$", tool("llvm-readelf", "-s", "--wide", elf), flags=re.M)
        ins, meta = instructions(elf), metadata(elf)
        for n in names:
            out[(base, n)] = (ins.get(n), meta.get(n))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "old"))
        os.makedirs(os.path.join(tmp, "new"))
        old = collect(sys.argv[1], os.path.join(tmp, "old"))
        new = collect(sys.argv[2], os.path.join(tmp, "new"))
    if not new:
        sys.exit("no gfx950 kernels under " + sys.argv[2])
    for key in sorted(new):
        obj, name = key
        if key not in old:
            print(f"differs: {name} ({obj}) is not in the old build")
            sys.exit(1)
        if not new[key][0] or new[key][0] != old[key][0]:
            print(f"differs: {name} ({obj}): instructions")
            sys.exit(1)
        if not new[key][1] or new[key][1] != old[key][1]:
            print(f"differs: {name} ({obj}): metadata {old[key][1]} -> {new[key][1]}")
            sys.exit(1)
    for obj, name in sorted(set(old) - set(new)):
        print(f"removed: {name} ({obj})")
    print(f"identical: {len(new)} kernels kept, {len(old) - len(new)} removed")


if __name__ == "__main__":
    main()
