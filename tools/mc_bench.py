"""Times marching cubes (ndjir_amd/mc.py, csrc/mc.hip) on an analytic G^3 volume at the size of a full extraction: a sphere of
radius 0.6 with a ripple, sampled on [-1, 1]^3 on the device.  Each pass runs once to warm up, then `repeats` times between a
host clock and a synchronise: the count pass with its scan (ndjir_mc_count), the emit pass (ndjir_mc_emit: vertices, then
faces) and the whole `marching_cubes` call (validation, the finiteness reduction, allocation and the one host wait included).
Prints one JSON line with the times in ms and the bytes each pass has to move.  Usage: mc_bench.py [repeats = 5] [G = 512]."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ndjir_amd import lib, mc

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
G = int(sys.argv[2]) if len(sys.argv) > 2 else 512
dev = torch.device("cuda:0")

ax = torch.linspace(-1, 1, G, device=dev)
vol = torch.empty((G, G, G), device=dev, dtype=torch.float32)
for i in range(G):          # slab by slab: no G^3 temporaries
    x, y, z = ax[i], ax[:, None], ax[None, :]
    vol[i] = torch.sqrt(x * x + y * y + z * z) - 0.6 + 0.02 * torch.sin(12 * x) * torch.sin(9 * y) * torch.cos(15 * z)


def timed(fn):
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


N = G ** 3
nb = -(-N // mc.SCAN_BLOCK)
table = mc._device_table(dev)
code = torch.empty(N, device=dev, dtype=torch.int16)
sums = torch.empty(2 * nb, device=dev, dtype=torch.int32)
counts = torch.empty(4, device=dev, dtype=torch.int32)
_, count_ms = timed(lambda: lib.call("mc_count", G, G, G, vol, 0.0, table, code, sums, counts))
V, F, over_v, over_f = counts.cpu().tolist()
assert not over_v and not over_f and V > 0
verts = torch.empty((V, 3), device=dev, dtype=torch.float32)
faces = torch.empty((F, 3), device=dev, dtype=torch.int32)
vertex_base = torch.empty(N, device=dev, dtype=torch.int32)
scale = [2.0 / (G - 1)] * 3
_, emit_ms = timed(lambda: lib.call("mc_emit", G, G, G, vol, 0.0, table, code, sums, scale, [-1.0] * 3, 0, vertex_base, verts, V,
                                    faces, F))
(v2, f2), total_ms = timed(lambda: mc.marching_cubes(vol, 0.0, "descent", [-1.0] * 3, [1.0] * 3))
assert torch.equal(v2, verts) and torch.equal(f2, faces)
# what the design has to move: per point, count reads 4 B of volume and writes the 2 B code; emit reads the code twice; plus
# block totals, per vertex its two samples, vertex_base and the row, per face the row and three (vertex_base, code) lookups
count_bytes = N * 6 + 2 * nb * 4 * 3
emit_bytes = N * 4 + 2 * nb * 4 + V * (8 + 4 + 12) + F * (12 + 3 * 6)
print(json.dumps(dict(G=G, vertices=V, faces=F, count_ms=count_ms, emit_ms=emit_ms, marching_cubes_ms=total_ms,
                      count_bytes=count_bytes, emit_bytes=emit_bytes,
                      count_GBps=count_bytes / (min(count_ms) * 1e-3) / 1e9, emit_GBps=emit_bytes / (min(emit_ms) * 1e-3) / 1e9)))
