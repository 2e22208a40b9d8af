"""Timing of the group catalogue on disk (mpg_dev_fof_save_groups) on the particles of bench.py's `fof` workload: n^3 (default 256^3) dark-matter
particles, a uniform background (60 %) plus Gaussian clumps of 20 .. 20000 members, linking length 0.2 mean separations, FOFHaloMinLength 32.
Usage: fof_catalogue_time.py [n] [repeats] [directory]   (directory: where the catalogues go, default /dev/shm, a tmpfs; each is removed again)
Reports, from the same run:
  mpg_dev_fof_fof       host clock around a device synchronise
  the catalogue         device times from events (mpg_fof_catalogue_get_times): the order (keys + radix sort), the sum of the gathers, the
                        FOFGroups scatters - separately from the file writes - and the end-to-end host time of the call into the directory
with the four bare-bone blocks (Mass, Position, Velocity, ID) plus GroupID of the one particle type, nfile 1."""
import importlib, math, os, shutil, sys, tempfile, time
sys.path.insert(0, '.')
import torch
pkg = importlib.import_module("mp-gadget_amd")
F = pkg.fof_catalogue
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
root = sys.argv[3] if len(sys.argv) > 3 else "/dev/shm"
dev = torch.device("cuda", 0)
N = n ** 3; box = 1000.0 * n; LL = 0.2 * box / n
g = torch.Generator(device=dev).manual_seed(7)
f8 = torch.float64
nback = int(0.6 * N)
parts = [torch.rand(nback, 3, dtype=f8, device=dev, generator=g) * box]
left = N - nback
cpu = torch.Generator().manual_seed(3)
while left > 0:
    m = min(left, int(torch.exp(torch.empty(1).uniform_(math.log(20.), math.log(20000.), generator=cpu)).item()))
    c = torch.rand(3, dtype=f8, device=dev, generator=g) * box
    parts.append(torch.remainder(c + torch.randn(m, 3, dtype=f8, device=dev, generator=g) * (0.25 * LL * m ** (1. / 3)), box))
    left -= m
pos = torch.cat(parts).contiguous(); pos.clamp_(min=1e-9)
mass = torch.ones(N, dtype=torch.float32, device=dev)
ids = torch.randperm(N, device=dev, generator=g).to(torch.int64)
vel = torch.randn(N, 3, dtype=f8, device=dev, generator=g)
grnr = torch.zeros(N, dtype=torch.int64, device=dev)
eng = pkg.Engine(0); eng.use_torch_stream()
eng.dev_bind_particles(pos, mass, box)
ng = eng.dev_fof_fof(ids, LL, 32, vel=vel, grnr=grnr); torch.cuda.synchronize()
ts = []
for _ in range(repeats):
    t0 = time.perf_counter(); ng = eng.dev_fof_fof(ids, LL, 32, vel=vel, grnr=grnr); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
ing = int((grnr >= 0).sum())
print("set: %d^3 = %d particles, box %g, %d groups, %d rows in groups (%.1f %%)" % (n, N, box, ng, ing, 100.0 * ing / N))
print("mpg_dev_fof_fof          min %.1f  median %.1f ms (%d calls)" % (min(ts), sorted(ts)[len(ts) // 2], repeats), flush=True)
cols = dict(Mass=mass, Position=pos, Velocity=vel, ID=ids)
rows = []
for k in range(repeats + 1):                                   # (the first call allocates the staging pair and rocPRIM's scratch: not reported)
    path = tempfile.mkdtemp(prefix="fofcat_", dir=root)
    t0 = time.perf_counter()
    F.save_fof_catalogue(eng, os.path.join(path, "PIG_000"), cols, 0.25, 1.0, CurrentParticleOffset=(0.25 * box, 0.0, 0.5 * box), ptypes=(1,), OutputPotential=0)
    wall = (time.perf_counter() - t0) * 1e3
    t = eng.fof_catalogue_times()
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(path) for f in fs)
    shutil.rmtree(path)
    if k:
        rows.append((wall, t["order_ms"], t["gather_ms"], t["group_ms"]))
rows.sort()
wall, o, ga, gr = rows[len(rows) // 2]
print("mpg_dev_fof_save_groups  median of %d calls into %s: %.1f ms end to end, %.1f MB written" % (repeats, root, wall, size / 1e6))
print("  device: order %.2f ms + gathers %.2f ms + FOFGroups blocks %.2f ms = %.2f ms; copies to the host and file writes: the other %.1f ms" %
      (o, ga, gr, o + ga + gr, wall - (o + ga + gr)))
print("  the columns a host-side writer would pull back first: %.1f MB (Position, Velocity, Mass, ID, GrNr of every row)" % (N * (24 + 24 + 4 + 8 + 8) / 1e6), flush=True)
eng.close()
