"""The PM step with the massive-neutrino linear response (and optionally the hybrid-neutrino deposit mask) on one GPU (mode "single")
or over the ranks through the library's choreography (mode "dist", csrc/dist.hip): mpg_dist_gravpm_force on each rank's particle
records, then mpg_dist_gravity_step on device arrays with the types set.  Rank 0 saves GravPM / Potential of the whole set, the
total-matter spectrum and what every rank's callback received.  Used by tests/test_gpu_nu_response.py; launch the dist mode with
torch.distributed.run (MPG_DIST_BACKEND=gloo lets the ranks share one GPU).  The env-selected transfer forms (MPG_PM_FUSE_PS=0,
MPG_PM_KSPACE_FORCE=1) are read once per process, which is why the single mode runs here too."""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("mp-gadget_amd")
import torch
import torch.distributed as dist

G = 43.0071


def synthetic_response(calls):
    """a stand-in for delta_nu_from_power built from its own inputs: ratio_i = 0.3 / (1 + (kk_i / kk[nonzero // 3])^2)"""
    def fn(kk, dcdm, nmodes):
        calls.append((kk.copy(), dcdm.copy(), nmodes.copy()))
        return np.log(kk), 0.3 / (1 + (kk / kk[len(kk) // 3]) ** 2), 0.07, 1.05
    return fn


def tracer_types(N):
    t = np.ones(N, np.uint8)
    t[::8] = 2
    return t


if __name__ == "__main__":
    out, n, nmesh = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    mode = os.environ.get("MPG_NU_MODE", "single")
    hybrid = os.environ.get("MPG_NU_HYBRID", "1") == "1"
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    lr = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(lr)
    dev = torch.device("cuda", lr)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29557")
        dist.init_process_group(os.environ.get("MPG_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    pos, mass, box = pkg.ics.s_zel(n)
    N = len(pos)
    types = tracer_types(N) if hybrid else np.ones(N, np.uint8)
    bmpc = box / 1000.0
    eng = pkg.Engine(lr)
    eng.use_torch_stream()
    eng.gravshort_fill_ntab(0, 1.5)
    eng.gravpm_init_periodic(box, 1.5, nmesh, G)
    eng.set_gravshort_treepar(TreeUseBH=0)
    eng.gravshort_set_softenings(box / n)
    calls = []
    eng.gravpm_set_hybrid_nu_tracer(hybrid)
    eng.gravpm_set_nu_response(synthetic_response(calls), bmpc)
    res = {}
    if mode == "single":
        P = pkg.make_particles(pos, mass, type=types)
        eng.gravpm_force(P)
        res["gravpm_host"], res["pot_host"] = P["GravPM"].copy(), P["Potential"].copy()
        kk, pw, nm = eng.gravpm_get_powerspectrum(nmesh, bmpc)
        # the device entry on bound arrays
        d_pos, d_mass = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev)
        d_type = torch.from_numpy(types).to(dev)
        eng.dev_bind_particles(d_pos, d_mass, box, type=d_type)
        g = torch.zeros(N, 3, dtype=torch.float64, device=dev)
        p = torch.zeros(N, dtype=torch.float64, device=dev)
        eng.dev_gravpm_force(g, p)
        torch.cuda.synchronize()
        res["gravpm_dev"], res["pot_dev"] = g.cpu().numpy(), p.cpu().numpy()
    else:
        DP = pkg.domain_peano
        share = slice((N * rank) // world, (N * (rank + 1)) // world)
        d_pos, d_mass = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev)
        ids = torch.arange(N, dtype=torch.int64, device=dev)[share]
        d_t = torch.from_numpy(types.astype(np.int64)).to(dev)
        dom = DP.PeanoDomain(eng, box, rank, world, overdecomposition=4)
        dom.decompose(d_pos[share].contiguous())
        opos, omass, oids, otype = dom.exchange(d_pos[share].contiguous(), d_mass[share].contiguous(), ids, d_t[share].contiguous())
        n_own = int(opos.shape[0])
        comm = pkg.dist.TorchComm(dev) if world > 1 else pkg.dist.LocalComm()
        df = pkg.dist.DistForce(eng, comm)
        df.set_domain(dom, 6.0 * 1.5 * box / nmesh)
        # 1. the drop-in form on the rank's particle records
        Prec = pkg.make_particles(opos.cpu().numpy(), omass.cpu().numpy(), type=otype.cpu().numpy().astype(np.uint8))
        df.host_gravpm_force(Prec)
        kk, pw, nm = df.gravpm_get_powerspectrum(nmesh, bmpc)
        f8 = dict(dtype=torch.float64, device=dev)
        # 2. gravity_step on device arrays, the types set for the deposit mask
        df.set_types(otype.to(torch.uint8).contiguous())
        ga, gg, gp = torch.zeros(n_own, 3, **f8), torch.zeros(n_own, 3, **f8), torch.zeros(n_own, **f8)
        df.gravity_step(opos, omass, ga, gg, potential=gp, oldacc=torch.full((n_own,), 1e-7, **f8))
        torch.cuda.synchronize()
        both = torch.zeros(N, 9, **f8)
        both[oids] = torch.cat([torch.from_numpy(Prec["GravPM"]).to(dev), torch.from_numpy(Prec["Potential"]).to(dev)[:, None], gg,
                                gp[:, None], torch.zeros(n_own, 1, **f8)], dim=1)
        if world > 1:
            pkg.rows.TargetExchange(world, dev).exchange(both, oids.to(torch.int32))
        b = both.cpu().numpy()
        res["gravpm_host"], res["pot_host"], res["gravpm_step"] = b[:, 0:3], b[:, 3], b[:, 4:7]
        df.close()
    # what this rank's callback received (one call per PM step)
    res["ncalls"] = np.array(len(calls))
    for i, (k, d, m) in enumerate(calls):
        res["call%d_kk" % i], res["call%d_dcdm" % i], res["call%d_nmodes" % i] = k, d, m
    res["ps_kk"], res["ps_P"], res["ps_N"] = kk, pw, nm
    np.savez(out + ".rank%d.npz" % rank, **res)
    eng.gravpm_set_nu_response(None)
    eng.close()
    if world > 1:
        dist.destroy_process_group()
    print("ok rank %d calls %d" % (rank, len(calls)), flush=True)
