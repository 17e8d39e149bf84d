# Storage of each level of a hierarchy on the GPU: the formats (sss_hip_level_info a_format / r_format /
# p_format bits), the bytes one SpMV streams of A_l (a_stream_bytes) and the level's slot of the byte
# ledger (sss_hip_cycle_bytes); then the ledger's outer-residual and coarse-solve slots, and the kernels
# of one captured cycle (sss_hip_cycle_launches, after one cycle from b = x = 1).
#   python tools/fmt_probe.py 64               7-pt 64^3
#   python tools/fmt_probe.py 27:16            27-pt 16^3
#   python tools/fmt_probe.py bus              tests/golden/1138_bus.mtx
#   python tools/fmt_probe.py 7:16 two-stage   ... with two-stage Jacobi on every level (the merged copies)
# Two builds of the library store a hierarchy alike iff their outputs are identical (SSS_AMG_LIB
# selects another build).
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import amg_amd as A
from conftest import build_hierarchy, quiet_ctx
what = sys.argv[1]
if what == "bus":
    with quiet_ctx():
        M = A.read_mtx(str(ROOT / "tests" / "golden" / "1138_bus.mtx"))
else:
    pts, _, n = what.rpartition(":")
    M = A.generate(int(pts or 7), int(n))
H = build_hierarchy(M, quiet_ctx)
kw = dict(smoother="hybrid", coarse="direct", sum_order=1)
if sys.argv[2:] == ["two-stage"]:
    kw = dict(smoother="jacobi", coarse="krylov", relabel=1, inner=1, inner_from=0, sum_order=1)
D = A.DeviceHierarchy(H, device=0, **kw)
cb = D.cycle_bytes()
for l in range(H.num_levels - 1):
    i = D.level_info(l); print(l, i.a_format, i.r_format, i.p_format, i.a_stream_bytes, int(cb["levels"][l]))
print("outer", int(cb["outer"]), "coarse", int(cb["coarse"]))
import numpy as np
D.upload(0, "b", np.ones(M.num_rows)); D.upload(0, "x", np.ones(M.num_rows))
D.cycle()   # captures the cycle: sss_hip_cycle_launches counts the kernels of the captured graph
print("launches", A.lib().sss_hip_cycle_launches(D.h))
