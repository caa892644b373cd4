#!/usr/bin/env python3
"""Developer tool: is the gfx950 device code of two engine libraries (or host objects) the same?  For refactors of the host side.

    python tools/cmp_device_code.py <lib A> <lib B>      exit status 0 = identical

Every gfx950 code object of every offload bundle is disassembled; required are the same set of function symbols and, for every
symbol, the same instruction listing (addresses and encodings left out, so the order of the functions inside a code object does
not count), and equal build.kernel_resources() -- registers, spills, LDS, scratch of every kernel.  A kernel that several translation
units emit (the re-spawn kernels, through hwy_launch.h) has one listing per code object: the SET of its distinct listings is what is
compared, so such a symbol is "the same" in two libraries exactly when every listing it has in one also occurs in the other --
two differing listings of one symbol inside a library are never folded into one, they make a set of two.  Needs no GPU."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from highwayenv_amd import build  # noqa: E402

OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-objdump")


def functions(path: str) -> dict:
    """symbol -> the sha256 of its instruction listing in every code object that defines it (sorted, duplicates folded)"""
    fns = {}
    for co in build.gfx950_code_objects(open(path, "rb").read()):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], capture_output=True, text=True,
                                 check=True).stdout
        name, body = None, []
        for line in txt.splitlines() + ["<end>:"]:
            m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
            if m:
                if name:  # (a kernel that several translation units emit: the set of its listings, one entry when they agree)
                    fns[name] = tuple(sorted(set(fns.get(name, ())) | {hashlib.sha256("\n".join(body).encode()).hexdigest()}))
                name, body = m.group(1), []
            elif name and line.strip() not in ("", "...") and not line.startswith("Disassembly of section"):  # ("...": padding)
                body.append(re.sub(r"\s*//.*$", "", line).strip())
    return fns


a, b = functions(sys.argv[1]), functions(sys.argv[2])
print(f"{len(a)} device functions in {sys.argv[1]}, {len(b)} in {sys.argv[2]}")
print("only in the first:", sorted(set(a) - set(b)))
print("only in the second:", sorted(set(b) - set(a)))
differ = sorted(k for k in a if k in b and a[k] != b[k])
print(f"{len(differ)} functions with a different instruction listing:", differ[:10])
ra, rb = build.kernel_resources(sys.argv[1]), build.kernel_resources(sys.argv[2])
print(f"kernel resources: {len(ra)} kernels against {len(rb)},", "equal" if ra == rb else
      f"DIFFERENT: {sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))[:10]}")
sys.exit(0 if set(a) == set(b) and not differ and ra == rb else 1)
