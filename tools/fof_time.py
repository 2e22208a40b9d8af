"""FOF timing experiments.  Without arguments: mpg_dev_fof_fof on uniform vs clumped sets of 256^3.
`subgrid [repeats]`: a 2 x 128^3 set of dark matter and gas in clumps, stars and black holes sprinkled in: the time of mpg_dev_fof_fof, of
mpg_dev_fof_subgrid and of mpg_dev_fof_seed (host clock around a device synchronise, after a warm-up call), and the bytes k_fof_subgrid has
to move, from the set's counts.  `fof [repeats]`: the same set, mpg_dev_fof_fof alone (runs on a tree without the sub-grid calls).
Kernel times: run either under a kernel trace (rocprofv3 --kernel-trace --stats) in a run of its own."""
import importlib, sys, time, math
sys.path.insert(0, '.')
import torch
pkg = importlib.import_module("mp-gadget_amd")
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(7)
f8 = torch.float64
def clumps(total, mmin, mmax, box, LL):
    parts, left = [], total
    cpu = torch.Generator().manual_seed(3)
    while left > 0:
        m = min(left, int(torch.exp(torch.empty(1).uniform_(math.log(mmin), math.log(mmax), generator=cpu)).item()))
        c = torch.rand(3, dtype=f8, device=dev, generator=g) * box
        parts.append(torch.remainder(c + torch.randn(m, 3, dtype=f8, device=dev, generator=g) * (0.25 * LL * m ** (1. / 3)), box))
        left -= m
    return torch.cat(parts)
def timed(fn, repeats):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return r, min(ts), sorted(ts)[len(ts) // 2], max(ts)
def subgrid_set(mode, repeats):
    n = 128; nd = n ** 3; N = 2 * nd; box = 1000.0 * n; LL = 0.2 * box / n
    rnd = lambda *s: torch.rand(*s, dtype=f8, device=dev, generator=g)
    dm = clumps(nd, 20, 20000, box, LL)
    gas = torch.remainder(dm + (rnd(nd, 3) - 0.5) * 0.2 * LL, box)                       # every gas row next to its dark-matter row
    pos = torch.cat([dm, gas]).contiguous(); pos.clamp_(min=1e-9)
    typ = torch.cat([torch.ones(nd, dtype=torch.uint8, device=dev), torch.zeros(nd, dtype=torch.uint8, device=dev)])
    u = rnd(N)
    typ[(typ == 0) & (u < 0.02)] = 4                                                    # 2 % of the gas rows are stars, 0.02 % black holes
    typ[(typ == 0) & (u > 0.9998)] = 5
    perm = torch.randperm(N, device=dev, generator=g)                                   # particle order is not type order
    pos, typ = pos[perm].contiguous(), typ[perm].contiguous()
    mass = torch.where(typ == 1, 0.8, 0.2).to(torch.float32)
    ids = torch.randperm(N, device=dev, generator=g).to(torch.int64)
    grnr = torch.zeros(N, dtype=torch.int64, device=dev)
    eng = pkg.Engine(0); eng.use_torch_stream()
    eng.dev_bind_particles(pos, mass, box, type=typ)
    ng, lo, med, hi = timed(lambda: eng.dev_fof_fof(ids, LL, 32, grnr=grnr), repeats)
    ingroup = grnr >= 0
    cnt = {t: int(((typ == t) & ingroup).sum()) for t in (0, 4, 5)}
    print("set: %d particles, %d groups, %d rows in groups (gas %d, stars %d, black holes %d)" % (N, ng, int(ingroup.sum()), cnt[0], cnt[4], cnt[5]))
    print("mpg_dev_fof_fof      min %.2f  median %.2f  max %.2f ms (%d calls)" % (lo, med, hi, repeats), flush=True)
    if mode == "fof":
        return
    cols = dict(sfr=rnd(N), metallicity=rnd(N) * 0.04, metals=(rnd(N, 9) * 0.01).to(torch.float32).contiguous(), heiii_ionized=(rnd(N) < 0.4).to(torch.uint8),
                bh_mass=rnd(N) * 1e-3, bh_mdot=rnd(N) * 1e-2, density=torch.exp(torch.randn(N, dtype=f8, device=dev, generator=g) * 3),
                delaytime=torch.where(rnd(N) < 0.3, 1.0, 0.0).to(f8))
    sub, lo, med, hi = timed(lambda: eng.dev_fof_subgrid(ng, WindDecouple=1, **cols), repeats)
    # what k_fof_subgrid reads: every row its place, group number and type (4 + 8 + 1), a row in a group the group's index (4); a gas row
    # Mass, Metallicity, Metals, Sfr, HeIIIionized, Density, DelayTime (4 + 8 + 36 + 8 + 1 + 8 + 8), a star row 4 + 8 + 36, a black hole 16
    nbytes = N * 13 + int(ingroup.sum()) * 4 + cnt[0] * 73 + cnt[4] * 48 + cnt[5] * 16
    print("mpg_dev_fof_subgrid  min %.3f  median %.3f  max %.3f ms (%d calls; with the allocation of its 10 output tensors)" % (lo, med, hi, repeats))
    print("k_fof_subgrid reads %.1f MB: divide by its kernel time from a trace for bytes/s; groups with a seed row %d" %
          (nbytes / 1e6, int((sub["seed_index"] >= 0).sum())))
    G = eng.dev_fof_groups(ng)
    par = pkg.engine.FofSeedParams(float(G["Mass"].median()), 0.2, 1e-4, 0.0, -2.0, 0.0)
    (parts, _, _), lo, med, hi = timed(lambda: eng.dev_fof_seed(par, 0.25, None), repeats)
    print("mpg_dev_fof_seed     min %.3f  median %.3f  max %.3f ms (%d calls; the list of %d seeds, two passes: its length, then the list)" %
          (lo, med, hi, repeats, len(parts)))
    # ... and with the conversion: the columns of blackhole_make_one, fresh for every call (a converted row is no gas any more)
    seedcols = lambda: dict(type=typ.clone(), mass=mass.clone(), bh_mass=torch.zeros(N, dtype=f8, device=dev), mtrack=torch.zeros(N, dtype=f8, device=dev),
                            minpotpos=torch.zeros(N, 3, dtype=f8, device=dev), countprogs=torch.zeros(N, dtype=torch.int32, device=dev))
    ts = []
    for _ in range(repeats + 1):
        c = seedcols(); torch.cuda.synchronize()
        t0 = time.perf_counter(); eng.dev_fof_seed(par, 0.25, c); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    ts = sorted(ts[1:])
    print("mpg_dev_fof_seed     min %.3f  median %.3f  max %.3f ms with k_blackhole_make_one on 6 columns" % (ts[0], ts[len(ts) // 2], ts[-1]), flush=True)
if len(sys.argv) > 1:
    subgrid_set(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    sys.exit(0)
n = 256; N = n ** 3; box = 1000.0 * n; LL = 0.2 * box / n
sets = {"uniform": lambda: torch.rand(N, 3, dtype=f8, device=dev, generator=g) * box,
        "clumps 20..20000": lambda: clumps(N, 20, 20000, box, LL),
        "clumps 20..200": lambda: clumps(N, 20, 200, box, LL),
        "4 clumps of 1M + uniform": lambda: torch.cat([clumps(4 << 20, 1 << 20, (1 << 20) + 1, box, LL), torch.rand(N - (4 << 20), 3, dtype=f8, device=dev, generator=g) * box])}
eng = pkg.Engine(0); eng.use_torch_stream()
for name, mk in sets.items():
    pos = mk().contiguous(); pos.clamp_(min=1e-9)
    mass = torch.ones(N, dtype=torch.float32, device=dev)
    ids = torch.randperm(N, device=dev, generator=g).to(torch.int64)
    grnr = torch.zeros(N, dtype=torch.int64, device=dev)
    eng.dev_bind_particles(pos, mass, box)
    ng = eng.dev_fof_fof(ids, LL, 32, grnr=grnr); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        ng = eng.dev_fof_fof(ids, LL, 32, grnr=grnr)
    torch.cuda.synchronize()
    print("%-18s %.1f ms  groups %d  in groups %d" % (name, (time.perf_counter() - t0) / 3 * 1e3, ng, int((grnr >= 0).sum())), flush=True)
