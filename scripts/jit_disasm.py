"""Disassembly of the plan-specialised af_flow_jit of `bench.py --config C` (no GPU needed): python scripts/jit_disasm.py C out.s
(prints the spec on stderr and one line of statistics: instructions by kind, registers, scratch bytes, spills)"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import bench  # noqa: E402
from asyncflow_amd import jit  # noqa: E402
from asyncflow_amd.engine import PLAN_ONLY, Engine  # noqa: E402

cfg = int(sys.argv[1])
args = bench.make_parser().parse_args(["--config", str(cfg)])
args.horizon = None
wl = bench.build_workload(cfg, 0, 1, 0, None)
shape = bench.rank_shape(wl, args)
eng = Engine(shape["plan"], PLAN_ONLY, **shape["engine_kw"])
hi = min(shape["slice"], shape["n"])
over = [(c, i, np.ascontiguousarray(v[:hi])) for c, i, v, _ in shape["over"]]
spec = eng.jit_spec(shape["seeds"][:hi], over, clock_ptr=8, clock_capacity=shape["clock_cap"], samples_ptr=8,
                    tick_capacity=shape["ticks"], counts_ptr=8, draw_capacity=shape["clock_cap"])
eng.close()
print(spec, file=sys.stderr)
image = jit.code_object(spec)
LLVM = "/opt/rocm/lib/llvm/bin/"
with tempfile.NamedTemporaryFile(suffix=".hsaco") as f, tempfile.NamedTemporaryFile(suffix=".elf") as elf:
    f.write(image)
    f.flush()
    subprocess.run([LLVM + "clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={f.name}",
                    f"--output={elf.name}", "--unbundle"], check=True)
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", elf.name], capture_output=True, text=True, check=True).stdout
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", elf.name], capture_output=True, text=True, check=True).stdout
Path(sys.argv[2]).write_text(dis)
# what an A/B of the kernel's source reports beside its time (profiles/r07/jit_disasm_c2_raw.txt): instructions of af_flow_jit
# by kind, and the registers / scratch of its metadata
body = re.search(r"^[0-9a-f]+ <af_flow_jit>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M).group(1)
ops = [ln.split()[0] for ln in body.splitlines() if re.match(r"\s+[a-z]", ln)]
meta = next((part for part in re.split(r"\n\s+- \.agpr_count", notes) if re.search(r"\.name:\s+af_flow_jit\b", part)), "")
print("insts", len(ops), *(f"{p} {sum(o.startswith(p) for o in ops)}" for p in ("v_", "v_readlane", "v_writelane", "v_xor_b32", "v_bitop3",
                                                                                "v_mad_u64_u32", "v_div_", "v_fma_f64", "scratch_")),
      *(f"{k} {' '.join(re.findall(re.escape(k) + ': +([0-9]+)', meta)) or '?'}"
        for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")))
