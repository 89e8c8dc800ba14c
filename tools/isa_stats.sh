#!/bin/bash
# Register / scratch / occupancy summary of every kernel of the library (gfx950), plus the .s for reading.
# Usage: tools/isa_stats.sh [extra hipcc flags...]   -> /tmp/isa/vpt.s
mkdir -p /tmp/isa
R=$(cd "$(dirname "$0")/.." && pwd)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math \
  -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -I"$R/volume_path_tracer_amd/csrc" \
  --cuda-device-only -S -o /tmp/isa/vpt.s "$@" "$R/volume_path_tracer_amd/csrc/vpt_gpu.hip" 2>&1 | grep -v "unused during compilation"
python3 - <<'PY'
import re, subprocess
t = open("/tmp/isa/vpt.s").read()
for m in re.finditer(r"^(_ZN3vpt\w+):\s*; @", t, re.M):
    seg = t[m.end():]
    get = lambda k: re.search(r"; %s: (\d+)" % k, seg).group(1)
    name = subprocess.run(["c++filt", "-p", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
    print(name.replace("vpt::", ""), "vgpr", get("NumVgprs"), "sgpr", get("NumSGPRsForWavesPerEU"), "lds", get("LDSByteSize"),
          "scratch", get("ScratchSize"), "occ", get("Occupancy"))
PY
