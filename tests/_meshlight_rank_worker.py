"""One rank of an N-rank run whose ranks SHARE a GPU, rendering with TRC_FLAG_MESH_LIGHTS: sample shards and sample groups x tile ranks
composed by trc_group_compose_samples[_async] / trc_group_allreduce_mean_accum, the collectives supplied through
trc_group_set_collectives (host-staged, gloo between the processes; RCCL refuses two ranks on one device).  Started by
tests/test_gpu_mesh_lights.py::test_sample_shards_compose_to_the_defined_frame; not a test module itself.

env: RANK, WORLD_SIZE (4), MASTER_ADDR, MASTER_PORT, TRC_ROOT, TRC_OUT (directory), TRC_MESH = ball | bigball
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.environ["TRC_ROOT"])
sys.path.insert(0, os.path.join(os.environ["TRC_ROOT"], "tests"))
import torch.distributed as dist  # noqa: E402

from tracer_amd import abi, host  # noqa: E402
from tracer_amd.device import Tracer  # noqa: E402
from tracer_amd.gloo_collectives import GlooCollectives  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    name, outdir = os.environ["TRC_MESH"], os.environ["TRC_OUT"]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    coll = GlooCollectives()
    out = {}
    W, H, spp = 96, 64, 16                             # test_gpu_mesh_lights.py: SHARD_W, SHARD_H, SHARD_SPP
    mesh = host.Mesh.ball(4, 6, 0.1) if name == "ball" else host.Mesh.ball(24, 24, 1.0)
    scene = host.HostScene(abi.SCENE_CORNELL_MESH, mesh)
    n = scene.view.n_index // 3
    tri = np.full(n, 4, np.uint32)                     # the red Lambert wall's material; six triangles the lamp's (material 3)
    tri[n // 3:n // 3 + 6] = 3
    MIS = abi.INTEGRATOR_MIS
    t = Tracer(0, hooks=True)                          # every rank on the same GPU
    t.upload_scene(scene.view); t.upload_triangle_materials(tri)
    t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
    t.set_collectives(coll, world, rank)
    # every rank its own sample group: the whole frame, spp / world samples from ITS seed, flag on
    t.clear_accum(); t.seed(abi.shard_seed(100, rank)); t.render(spp=spp // world, integrator=MIS, mesh_lights=True)
    out["own"] = t.download_accum()
    out["n_lights"] = np.array(t.mesh_light_tables(n)["n_lights"])
    t.group_compose_samples(0)
    if rank == 0:
        out["samples"] = t.download_composed()
    t.group_allreduce_mean_accum()
    out["mean"] = t.download_accum()
    # S = 2 sample groups x T = 2 tile ranks, pipelined
    S, T = world // 2, 2
    t.synchronize(); t.clear_accum(); t.seed(abi.shard_seed(200, rank // T))
    t.render(spp=spp // S, integrator=MIS, mesh_lights=True, tile_rank=rank % T, tile_nranks=T)
    t.group_compose_samples_async(0, S)
    if rank == 0:
        out["hybrid"] = t.download_composed()
    t.synchronize()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    t.group_finalize()
    dist.barrier()
    dist.destroy_process_group()
    t.close()


if __name__ == "__main__":
    main()
