"""The communicator callbacks the multi-rank layer (csrc/dist*.hip, mpg_dist_*) makes, pinned call by call: ONE rank behind a recording
communicator - a Python mpg_comm whose callbacks copy to self, as world size 1 allows, and append (callback, counts or bytes, on_device)
to a list - drives a seeded scene of 4096 particles (16^3 Zel'dovich, a quarter of them gas, Nmesh 16) through

    domain_decompose, domain_exchange, use_decomposition, gravity_step, grav_short_tree with an active list,
    grav_short_tree_active_tree, force_tree_build, density and hydro_force (whole, then with an active list), fof_fof,
    gravpm_get_powerspectrum, potential_planes

and the sequence recorded for every call must equal tests/golden/dist_collectives.json, which this file wrote once
(`python tests/test_gpu_dist_collectives.py --record`) from the build of the commit before the layer was split into files.  The multi-rank
tests can show an added, dropped or reordered collective only by hanging; this one shows it as a difference of two lists.

Two communicators: "host" (device_buffers = 0: the library stages every exchange through pinned host memory) and "stream"
(device_buffers = 1 with bind_stream: the callbacks get device pointers and are queued on the engine's stream, which is torch's current
stream here, so the callback's copy is ordered with the library's work; bind_stream itself is recorded).  What is recorded: allreduce
(count, dtype, op), alltoall_i64 (the count sent), alltoallv (bytes and displacements sent and received), bind_stream ().  With one
rank and callbacks present every exchange goes through them; only the host all-gathers of blocks (allgather_host, the group records of
FOF) and the plane sums short-cut at NTask == 1, so potential_planes records nothing - which is pinned as well."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dist_collectives.json")
MODES = ("host", "stream")


class RecordingComm:
    """mpg_comm of one rank: every callback copies to self and is appended to .log"""

    def __init__(self, D, device, on_device):
        self.D, self.device, self.dev_bufs = D, device, bool(on_device)
        self.rank, self.world, self.errors, self.log = 0, 1, [], []
        self._fns = (D.ALLREDUCE_FN(self._allreduce), D.A2A_I64_FN(self._alltoall_i64), D.A2AV_FN(self._alltoallv),
                     D.BIND_STREAM_FN(self._bind_stream) if on_device else D.BIND_STREAM_FN())   # keep alive
        self.struct = D.MpgComm(None, 0, 1, 1 if on_device else 0, *self._fns)

    def _guard(self, f):
        try:
            f()
            return 0
        except Exception as e:      # a callback must not raise through the C frames
            self.errors.append(repr(e))
            return 1

    def _allreduce(self, ctx, buf, count, dtype, op, on_device):
        return self._guard(lambda: self.log.append(["allreduce", [int(count), int(dtype), int(op)], int(on_device)]))   # (the sum over one rank)

    def _alltoall_i64(self, ctx, send, recv):
        def go():
            recv[0] = send[0]
            self.log.append(["alltoall_i64", [int(send[0])], 0])
        return self._guard(go)

    def _alltoallv(self, ctx, send, sbytes, sdispls, recv, rbytes, rdispls, on_device):
        def go():
            n = int(sbytes[0])
            self.log.append(["alltoallv", [n, int(sdispls[0]), int(rbytes[0]), int(rdispls[0])], int(on_device)])
            assert n == int(rbytes[0]) and n >= 0
            if n == 0:
                return
            src, dst = int(send) + int(sdispls[0]), int(recv) + int(rdispls[0])
            if on_device:
                self.D._bytes_tensor(dst, n, True, self.device).copy_(self.D._bytes_tensor(src, n, True, self.device))
            else:
                C.memmove(dst, src, n)
        return self._guard(go)

    def _bind_stream(self, ctx, stream):
        return self._guard(lambda: self.log.append(["bind_stream", [], 1]))


def run_scene(pkg, mode):
    """the whole sequence behind one recording communicator: call -> the callbacks it made"""
    import torch
    D = pkg.dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    keep_stream = torch.cuda.current_stream()
    n, nmesh = 16, 16
    pos, mass, box = pkg.ics.s_zel(n, box=8.0)
    N = len(pos)
    rng = np.random.RandomState(3)
    typ = np.ones(N, np.uint8)
    typ[rng.choice(N, N // 4, replace=False)] = 0
    vel = rng.standard_normal((N, 3))
    ent = 1.0 + 0.5 * rng.random_sample(N)
    ids = (rng.permutation(N) + 1000).astype(np.int64)
    f8 = dict(dtype=torch.float64, device=dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eng = pkg.Engine(0)
    eng.use_torch_stream()
    eng.gravshort_fill_ntab(0, 1.5)
    eng.gravpm_init_periodic(box, 1.5, nmesh, 43.0071)
    eng.gravpm_measure_power(True)
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(box / n)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_hydropar(0, 100.0, 0.75)
    t = pkg.SphTimes()
    t.atime, t.hubble = 0.5, 0.3
    for i in range(47):
        t.dloga_bin[i] = 0.01
    comm = RecordingComm(D, dev, mode == "stream")
    out = {}

    def call(name, fn):
        start = len(comm.log)
        r = fn()
        assert not comm.errors, comm.errors
        out[name] = comm.log[start:]
        return r

    df = call("create", lambda: D.DistForce(eng, comm))
    margin = 3.5          # >= Rcut = 4.5 Asmth cells of 0.5 and >= the smoothing lengths and 6.4 linking lengths below; level La = 1
    g_pos = T(pos)
    call("domain_decompose", lambda: df.domain_decompose(g_pos, box))
    o_pos, o_mass, o_typ, o_vel, o_ent, o_ids = call("domain_exchange", lambda: df.domain_exchange(g_pos, T(mass), T(typ), T(vel), T(ent), T(ids)))
    assert o_pos.shape[0] == N
    call("use_decomposition", lambda: df.use_decomposition(box, margin))
    acc, gpm, pot = torch.zeros(N, 3, **f8), torch.zeros(N, 3, **f8), torch.zeros(N, **f8)
    call("gravity_step", lambda: df.gravity_step(o_pos, o_mass, acc, gpm, potential=pot))
    act = torch.arange(0, N, 3, dtype=torch.int32, device=dev)
    call("grav_short_tree_active", lambda: df.grav_short_tree(acc, prev_accel=acc.clone(), gravpm=gpm, active=act))
    a_pos, a_mass = o_pos[act.long()].contiguous(), o_mass[act.long()].contiguous()
    a_acc = torch.zeros(a_pos.shape[0], 3, **f8)
    call("grav_short_tree_active_tree", lambda: df.grav_short_tree_active_tree(a_pos, a_mass, a_acc))
    call("force_tree_build", lambda: df.force_tree_build(o_pos, o_mass))
    z1 = lambda: torch.zeros(N, **f8)
    a = dict(hsml=torch.full((N,), 2.2 * box / n, **f8), dthsml=z1(), vel=o_vel.contiguous(), entropy=o_ent.contiguous(), density=z1(), egywtdensity=z1(),
             dhsmlegyfac=z1(), divvel=z1(), curlvel=z1(), hydroacc_out=torch.zeros(N, 3, **f8), dtentropy_out=z1(), maxsignalvel=z1())
    call("density", lambda: df.density(o_typ, a, t))
    call("hydro_force", lambda: df.hydro_force(N, a, t))
    call("density_active", lambda: df.density(o_typ, a, t, active=act))
    call("hydro_force_active", lambda: df.hydro_force(N, a, t, active=act))
    call("fof_fof", lambda: df.fof_fof(o_pos, o_mass, o_ids, 0.2 * box / n, 8, type=o_typ, vel=o_vel.contiguous()))
    call("gravpm_get_powerspectrum", lambda: df.gravpm_get_powerspectrum(nmesh, box))
    call("potential_planes", lambda: df.potential_planes(o_pos, box, 16, [0, 1, 2], mass=o_mass, atime=0.5, comoving_distance=2.5e5, HubbleParam=0.7,
                                                         omega_source=0.27))
    torch.cuda.synchronize()
    df.close()
    eng.close()
    torch.cuda.set_stream(keep_stream)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", MODES)
def test_collectives_per_call(pkg, golden, mode):
    got = run_scene(pkg, mode)
    want = golden[mode]
    for name in want:
        print(mode, name, len(got.get(name, [])), "callbacks")
    assert list(got) == list(want), "the calls of the scene"
    for name in want:
        assert got[name] == want[name], "%s / %s: the sequence of communicator callbacks differs from the recorded one" % (mode, name)
    assert {c[0] for v in want.values() for c in v} >= {"allreduce", "alltoall_i64", "alltoallv"}    # (the record holds all three collectives)


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, ROOT)
    rec = {m: run_scene(importlib.import_module("mp-gadget_amd"), m) for m in MODES}
    path = sys.argv[sys.argv.index("--record") + 1] if "--record" in sys.argv and len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": {\n' % m + ",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in rec[m].items()) + "\n }" for m in MODES) + "\n}\n")
    print({m: {k: len(v) for k, v in rec[m].items()} for m in MODES})
