"""Times the vertex-attribute baking of the mesh export (ndjir_amd/extract.py::bake_vertex_attributes;
python/extract_by_mc.py:144-216) through the default.yaml networks (512^3 x 4 voxel grid): N points drawn uniformly in the
bounding box, the six textures, the normal and the sdf for each.  Usage: bake_bench.py [N = 2^20] [chunk = 2^18] [repeats = 3]."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ndjir_amd import config, network, parameter as P
from ndjir_amd.extract import bake_vertex_attributes

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 18
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = torch.device("cuda:0")
conf = config.load("default")
P.clear_parameters(); P.set_device(dev); network.seed(313)
gen = torch.Generator(device=dev)
gen.manual_seed(7)
pts = torch.rand((N, 3), device=dev, generator=gen) * 2 - 1
bake_vertex_attributes(pts[:min(N, 2 * chunk)], conf, chunk=chunk)        # warm-up: parameters, weight packing, allocator, the timed shapes
torch.cuda.synchronize()
times = []
for _ in range(repeats):
    t0 = time.perf_counter()
    out = bake_vertex_attributes(pts, conf, chunk=chunk)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
el = min(times)
print(json.dumps({"points": N, "chunk": chunk, "seconds": el, "seconds_all": times, "points_per_s": N / el,
                  "finite": bool(all(torch.isfinite(t).all() for t in out.values())),
                  "std_max": [float(out[k].max()) for k in ("roughness_std", "specular_reflectance_std")]}))
