#!/usr/bin/env python3
"""Per-kernel disassembly diff of the gfx950 code object inside two builds of one object file (e.g. cor_amd/csrc/build/retrieval.o of
the parent commit and of this one): the check that a change which adds template flavours leaves every existing kernel
instruction-for-instruction as it was.
    python tools/kernel_disasm_diff.py PARENT.o NEW.o [--rename [NAMES:]FROM=TO ...]
--rename maps a parent symbol onto its new name when a template gained a defaulted parameter (the mangled name grows, the code must
not); NAMES (comma-separated substrings) limits it to the symbols that contain one of them. For sim_scan / sim_wide_scan gaining
`bool GROUP = false`:  --rename sim_scan,sim_wide_scan:EEEvPK=ELb0EEEvPK
The literal of the s_add_u32 behind an s_getpc_b64 (the pc-relative address of a callee or a global) is masked: it moves with the size of
every other function in the code object, not with the function's own code.
Needs llvm-objcopy, clang-offload-bundler and llvm-objdump from ROCm's LLVM. Exit status 1 if a parent kernel is missing or differs."""
import os, re, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def kernels(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}",
                    "--unbundle"], check=True)
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True,
                          text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^\S*<(.+)>:\s*$", line)
        if m:
            cur = m.group(1); out[cur] = []
        elif cur is not None and line.strip() and line.strip() != "...":      # "...": zero padding up to the next symbol
            insn = re.sub(r"//.*$", "", line).strip()
            if insn.startswith("s_add_u32") and out[cur] and out[cur][-1].startswith("s_getpc_b64"):
                insn = re.sub(r"0x[0-9a-f]+$", "<pcrel>", insn)
            out[cur].append(insn)
    return out


def main():
    args = sys.argv[1:]
    renames = []
    while "--rename" in args:
        i = args.index("--rename"); spec = args[i + 1]; del args[i:i + 2]
        only, _, pair = spec.rpartition(":")
        a, b = pair.split("=")
        renames.append((only.split(",") if only else None, a, b))
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(args[0], tmp, "old"), kernels(args[1], tmp, "new")
    same, bad, mapped = 0, 0, set()
    for name, code in old.items():
        n = name
        for only, a, b in renames:
            if only is None or any(o in name for o in only):
                n = n.replace(a, b, 1)
        mapped.add(n)
        if n not in new:
            print("MISSING", name); bad += 1
        elif new[n] != code:
            print("DIFFERENT", name, len(code), len(new[n])); bad += 1
        else:
            same += 1
    print(f"{len(old)} parent kernels: {same} identical, {bad} missing or different; {len(set(new) - mapped)} kernels only in the new build")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
