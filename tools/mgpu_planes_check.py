"""The lensing potential planes over the ranks (mpg_dist_potential_planes, csrc/dist.hip): every rank takes the rows rank::world of
ics.s_zel(n) plus a few appended edge particles, and calls the collective with three cut points and the three normals.  Each rank saves
the planes and npart it received and the sum over the ranks of its own counters (mpg_dev_plane_counts, summed here with the process
group).  MPG_PLANES_NU=1: the call is made with a correction callback and must be refused on every rank before any collective; the
message is saved instead.  MPG_PLANES_BUDGET=1: rank r allows itself the counters of r + 2 planes, so the ranks must agree on a batch.
MPG_PLANES_BAD_ROW=1: rank 0 holds one position that is not finite; every rank must return the refusal.  Used by tests/test_gpu_planes.py; launch with torch.distributed.run (MPG_DIST_BACKEND=gloo lets the ranks share
one GPU)."""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("mp-gadget_amd")
import torch
import torch.distributed as dist

COSMO = dict(atime=0.5, comoving_distance=2.5e5, HubbleParam=0.7, omega_source=0.27)


def particle_set(n):
    """s_zel(n) and particles at coordinates exactly 0 and Box"""
    pos, mass, box = pkg.ics.s_zel(n)
    edge = np.array([[0.0, 0.3 * box, 0.6 * box], [box, 0.3 * box, 0.6 * box], [0.2 * box, 0.0, box], [0.7 * box, box, 0.0]])
    return np.concatenate([pos, edge]), np.concatenate([mass, np.full(len(edge), mass[0], mass.dtype)]), box


def plane_args(box):
    return dict(Thickness=0.3 * box, CutPoints=[0.35 * box, 0.05 * box, 0.9 * box], CurrentParticleOffset=(0.1 * box, 0.0, -0.25 * box), **COSMO)


if __name__ == "__main__":
    out, n, R = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    with_nu = os.environ.get("MPG_PLANES_NU", "0") == "1"
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    lr = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(lr)
    dev = torch.device("cuda", lr)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29557")
        dist.init_process_group(os.environ.get("MPG_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    pos, mass, box = particle_set(n)
    eng = pkg.Engine(lr)
    eng.use_torch_stream()
    comm = pkg.dist.TorchComm(dev) if world > 1 else pkg.dist.LocalComm()
    df = pkg.dist.DistForce(eng, comm)
    d_pos = torch.from_numpy(np.ascontiguousarray(pos[rank::world])).to(dev)
    d_mass = torch.from_numpy(np.ascontiguousarray(mass[rank::world])).to(dev)
    res = {}
    kw = plane_args(box)
    if os.environ.get("MPG_PLANES_BUDGET", "0") == "1":
        eng.set_plane_counter_budget((rank + 2) * R * R * 12)
    if os.environ.get("MPG_PLANES_BAD_ROW", "0") == "1":
        if rank == 0:
            d_pos[3, 1] = float("inf")
        try:
            df.potential_planes(d_pos, box, R, [0, 1, 2], mass=d_mass, **kw)
            res["error"] = np.array("")
        except pkg.EngineError as e:
            res["error"] = np.array(str(e))
    elif with_nu:
        eng.gravpm_init_periodic(box, 1.5, 32, 43.0071)
        try:
            df.potential_planes(d_pos, box, R, [0, 1, 2], mass=d_mass, nu_response=lambda k, d, m: (np.log(k), np.zeros_like(k), 0.0, 1.0),
                                BoxSize_in_MPC=box / 1000.0, **kw)
            res["error"] = np.array("")
        except pkg.EngineError as e:
            res["error"] = np.array(str(e))
    else:
        planes, npart = df.potential_planes(d_pos, box, R, [0, 1, 2], mass=d_mass, **kw)
        counts, nact = eng.dev_plane_counts(R, [0, 1, 2], **kw)
        torch.cuda.synchronize()
        c64 = counts.to(torch.int64).cpu()
        na = torch.tensor([nact], dtype=torch.int64)
        if world > 1:
            dist.all_reduce(c64)
            dist.all_reduce(na)
        res.update(planes=planes.cpu().numpy(), npart=npart, counts=c64.numpy(), n_active=na.numpy())
    np.savez(out + ".rank%d.npz" % rank, **res)
    df.close()
    eng.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("ok rank %d" % rank, flush=True)
