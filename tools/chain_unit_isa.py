"""Static per-unit ISA report of the token-ring chain kernel (af_ring_kernel.hip); needs hipcc, no GPU.

    python tools/chain_unit_isa.py [--kernel 16,4,false] [--asm FILE.s] [--json]

Compiles af_ring_kernel.hip to gfx950 assembly with the Makefile's flags (or reads a listing made by `make asm`), cuts each
instantiation of `chain_ring_kernel` at the serial units' edges (the `;;#af-unit-begin/end <token>` comments token_wait and
token_pass leave in the listing) and counts, per unit: instructions, f64 instructions, scratch loads / stores, v_readlane
(spilled SGPRs come back through VGPR lanes), LDS ops, global loads and f64 divisions (v_div_fixup_f64).  A unit appears
once per chunk body the kernel instantiates (full chunk first, then the guarded partial chunk) and once per copy LLVM makes;
every copy is listed.  These are static counts: a branch inside a unit that is not taken on every chunk counts as if it were.
Kernel-wide register use and spills come from the compiler's resource-usage remarks."""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-forge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the Makefile's CXXFLAGS (make asm)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]
# token numbers of af_ring_kernel.hip (enum kTokIn ...)
UNIT_NAMES = {"0": "input", "1": "sidechain(A)", "2": "peak-envelope(C)", "3": "gain-smoothing(E)", "4": "meter",
              "5": "limiter", "6": "true-peak", "7": "final-fold", "eq": "eq-group"}
COUNTERS = {
    "insts": None,
    "f64": re.compile(r"_f64\b|_b64_e32|_f64_e32|_f64_e64"),
    "scratch_load": re.compile(r"^\s*scratch_load"),
    "scratch_store": re.compile(r"^\s*scratch_store"),
    "readlane": re.compile(r"^\s*v_readlane"),
    "lds": re.compile(r"^\s*ds_"),
    "global_load": re.compile(r"^\s*global_load"),
    "div_f64": re.compile(r"^\s*v_div_fixup_f64"),
}
INST = re.compile(r"^\s+[a-z][a-z0-9_]*(\s|$)")


def compile_asm(out_path: str) -> str:
    cmd = [HIPCC, "--offload-arch=gfx950", *FLAGS, "-x", "hip", os.path.join(CSRC, "af_ring_kernel.hip"), "-S",
           "--cuda-device-only", "-o", out_path, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"hipcc failed ({r.returncode})")
    return r.stderr


def resource_usage(remarks: str) -> dict:
    """{mangled kernel name: {field: value}} from -Rpass-analysis=kernel-resource-usage."""
    out: dict = {}
    cur = None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?):\s*(\S+)\s*\[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def mangled(spec: str) -> str:
    w, c, auto = spec.split(",")
    return f"_ZN2af17chain_ring_kernelILi{int(w)}ELi{int(c)}ELb{1 if auto.strip().lower() in ('1', 'true', 'auto') else 0}EEEvNS_10LaunchArgsEPKNS_11ChainParamsE"


def function_body(lines: list[str], name: str) -> list[str]:
    start = next((i for i, l in enumerate(lines) if l.startswith(name + ":")), None)
    if start is None:
        raise SystemExit(f"{name} not in the listing")
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    # blocks LLVM placed after s_endpgm still belong to the function: up to its .Lfunc_end label
    fend = next((i for i in range(end, len(lines)) if lines[i].startswith(".Lfunc_end")), end)
    return lines[start:fend + 1]


def count(seg: list[str]) -> dict:
    c = {k: 0 for k in COUNTERS}
    for l in seg:
        if not INST.match(l) or l.lstrip().startswith(";"):
            continue
        c["insts"] += 1
        op = l.split()[0]
        for k, rx in COUNTERS.items():
            if rx is None:
                continue
            if k == "f64":
                c[k] += 1 if rx.search(op) else 0
            elif rx.match(l):
                c[k] += 1
    return c


def units(body: list[str]) -> list[dict]:
    out, open_ = [], None
    for i, l in enumerate(body):
        m = re.search(r";;#af-unit-(begin|end) (\S+)", l)
        if not m:
            continue
        kind, tok = m.groups()
        if kind == "begin":
            open_ = (tok, i)
        elif open_ is not None and open_[0] == tok:
            seg = body[open_[1] + 1:i]
            out.append({"token": tok, "unit": UNIT_NAMES.get(tok, tok), "line": open_[1], **count(seg)})
            open_ = None
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--kernel", default="16,4,false", help="waves,chunk,auto (default 16,4,false: the bench's kernel)")
    ap.add_argument("--asm", default=None, help="read this listing instead of compiling (resource usage is then omitted)")
    ap.add_argument("--json", action="store_true", help="print one JSON object instead of the table")
    args = ap.parse_args()
    if args.asm:
        text, remarks = open(args.asm).read(), ""
    else:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "af_ring_kernel.s")
            remarks = compile_asm(path)
            text = open(path).read()
    name = mangled(args.kernel)
    body = function_body(text.splitlines(), name)
    rows = units(body)
    usage = resource_usage(remarks).get(name, {})
    total = count(body)
    if args.json:
        print(json.dumps({"kernel": f"chain_ring_kernel<{args.kernel}>", "resource_usage": usage, "kernel_totals": total,
                          "units": rows}))
        return 0
    print(f"chain_ring_kernel<{args.kernel}>")
    if usage:
        print("  " + ", ".join(f"{k} {usage[k]}" for k in ("VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill",
                                                         "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]") if k in usage))
    print(f"  whole kernel: " + ", ".join(f"{k} {v}" for k, v in total.items()))
    cols = list(COUNTERS)
    print(f"  {'unit':20s} {'copy':>4s} " + " ".join(f"{c:>13s}" for c in cols))
    seen: dict = {}
    for r in rows:
        seen[r["unit"]] = seen.get(r["unit"], 0) + 1
        print(f"  {r['unit']:20s} {seen[r['unit']]:4d} " + " ".join(f"{r[c]:13d}" for c in cols))
    return 0


if __name__ == "__main__":
    sys.exit(main())
