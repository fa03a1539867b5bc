"""Where do the waves of the UCT headline launch finish?  (profiles/uct_wave_balance.md)

Needs a library built with the wave stamps compiled in (a diagnostic build: no stamp executes in the plain one):

    MP_EXTRA_FLAGS=-DMP_WAVE_STAMPS python -m rl_agents_amd.build --force      # (or into another directory: MI355PLAN_LIB)
    MI355PLAN_NO_TORCH=1 python tools/uct_wave_finish.py [n_roots] [launches]
    MP_UCT_BALANCE=0 ... the same                                              # the schedule without the wave balance

Lane 0 of every wave of uct_kernel stores the 100 MHz constant clock at entry, after the staging barrier, after its last episode
and at exit, with HW_ID and XCC_ID; the library writes the stamps of each launch to the file MP_UCT_WAVE_STAMPS names.  This tool
runs the headline launch (highway table 10 x 10 x 100, 262 144 roots, 33 episodes x 30 steps), takes the stamps of the last
launch and prints, as shares of the kernel (first entry to last exit):
  * the finish time by AGE RANK within the SIMD (the order of the entry stamps among the waves of one workgroup on one SIMD), per XCD;
  * the spread of finish times within SIMDs against the spread across SIMDs of a CU, across CUs and across XCDs;
  * the launch ramp (entry stamps), the staging time (entry to barrier), the read-out (last episode to exit) and the mean wave
    lifetime.
One tick is 10 ns, 0.002 of a 0.5 ms kernel.
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MI355PLAN_NO_TORCH", "1")
os.environ.setdefault("MP_PIPE_CHUNK", "0")      # host arrays, but ONE launch of all roots as bench.py's device call makes it: no chunks


def read_stamps(path):
    raw = np.fromfile(path, dtype=np.uint64)
    waves_per_wg, words = int(raw[0]), int(raw[1])
    return waves_per_wg, raw[2:].reshape(-1, words)


def analyse(waves_per_wg, st, out=sys.stdout):
    def show(*a):
        print(*a, file=out)
    entry, staged, done, exit_ = (st[:, k].astype(np.int64) for k in range(4))
    planned = done > staged                     # (a wave without roots stamps the three at once)
    hw, xcc = (st[:, 4] & 0xffffffff).astype(np.int64), (st[:, 4] >> 32).astype(np.int64) & 0xf
    simd, cu, sh, se = (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
    wg = np.arange(len(st)) // waves_per_wg
    t0, t1 = entry.min(), exit_.max()
    T = float(t1 - t0)
    fin = (exit_ - t0) / T
    show("waves {} ({} per workgroup, {} planning), kernel {:.1f} us (first entry to last exit)".format(
        len(st), waves_per_wg, int(planned.sum()), T / 100.0))
    show("mean wave lifetime / kernel: {:.3f}   launch ramp (entry stamps, last - first): {:.1f} us".format(
        float(((exit_ - entry) / T).mean()), (entry.max() - t0) / 100.0))
    show("staging (entry -> barrier): mean {:.2f} us, max {:.2f} us; read-out (last episode -> exit): mean {:.2f} us, max {:.2f} us".format(
        float((staged - entry).mean()) / 100.0, float((staged - entry).max()) / 100.0, float((exit_ - done)[planned].mean()) / 100.0,
        float((exit_ - done)[planned].max()) / 100.0))
    cu_key = ((xcc * 8 + se) * 2 + sh) * 16 + cu
    wgs_per_cu = len(set(zip(cu_key.tolist(), wg.tolist()))) / float(len(set(cu_key.tolist())))
    show("CUs used {}, workgroups per CU {:.2f}".format(len(set(cu_key.tolist())), wgs_per_cu))
    # groups: the planning waves of one workgroup on one SIMD, ranked by entry stamp (ties: by wave number)
    groups = {}
    for i in np.flatnonzero(planned):
        groups.setdefault((int(wg[i]), int(simd[i])), []).append(i)
    sizes = np.bincount([len(g) for g in groups.values()])
    show("waves of a workgroup per SIMD: " + ", ".join("{} SIMDs x {}".format(n, k) for k, n in enumerate(sizes) if n))
    top = max(len(g) for g in groups.values())
    by_rank = {}                                  # (xcc, size, rank) -> finish shares
    within, first_in_simd, last_in_simd = [], [], []
    for (g_wg, g_simd), idx in groups.items():
        idx = sorted(idx, key=lambda i: (entry[i], i))
        f = fin[idx]
        for rank, i in enumerate(idx):
            by_rank.setdefault((int(xcc[i]), len(idx), rank), []).append(fin[i])
        if len(idx) >= 2:
            within.append(f.max() - f.min())
        first_in_simd.append(f.min())
        last_in_simd.append(f.max())
    # the tail: from the moment the first SIMD has no episode left to run (the last of its waves stamped `done`) to the last exit
    simd_done = [max(done[i] for i in idx) for idx in groups.values()]
    last_wave = [max(idx, key=lambda i: exit_[i]) for idx in groups.values()]
    show("first SIMD out of episodes at {:.3f} of the kernel: {:.3f} of it ({:.1f} us) lies behind; read-out of the last wave of a "
         "SIMD: mean {:.2f} us".format((min(simd_done) - t0) / T, (t1 - min(simd_done)) / T, (t1 - min(simd_done)) / 100.0,
                                       float(np.mean([exit_[i] - done[i] for i in last_wave])) / 100.0))
    show("\nfinish time (share of the kernel) by age rank within the SIMD, SIMDs that hold {} waves; rank 0 entered first".format(top))
    show("  XCD   " + "  ".join("rank {}".format(k) for k in range(top)) + "    SIMDs")
    for x in sorted(set(xcc.tolist())) + [-1]:
        cells, n = [], 0
        for k in range(top):
            v = [u for (xx, size, rank), vals in by_rank.items() if size == top and rank == k and (x < 0 or xx == x) for u in vals]
            n = len(v)
            cells.append("{:.3f}".format(np.mean(v)) if v else "  -  ")
        show("  {:>3}   ".format("all" if x < 0 else x) + "   ".join(cells) + "    {}".format(n))
    show("\nspread of finish times (shares of the kernel)")
    if within:
        show("  within a SIMD (last - first of its waves): mean {:.3f}, median {:.3f}, max {:.3f}".format(
            float(np.mean(within)), float(np.median(within)), float(np.max(within))))
    show("  first wave of a SIMD to finish: mean {:.3f}; last wave of a SIMD: mean {:.3f}, min {:.3f}, max 1.000".format(
        float(np.mean(first_in_simd)), float(np.mean(last_in_simd)), float(np.min(last_in_simd))))
    cu_last, cu_mean = {}, {}
    for i in np.flatnonzero(planned):
        cu_last[int(cu_key[i])] = max(cu_last.get(int(cu_key[i]), 0.0), fin[i])
        cu_mean.setdefault(int(cu_key[i]), []).append(fin[i])
    cl = np.array(list(cu_last.values()))
    cm = np.array([np.mean(v) for v in cu_mean.values()])
    show("  across CUs: last wave of a CU min {:.3f} / mean {:.3f} / max {:.3f}; mean finish of a CU min {:.3f} / max {:.3f}".format(
        cl.min(), cl.mean(), cl.max(), cm.min(), cm.max()))
    xs = sorted(set(xcc.tolist()))
    show("  across XCDs: mean finish " + " ".join("{}:{:.3f}".format(x, float(fin[planned & (xcc == x)].mean())) for x in xs))
    show("               last exit   " + " ".join("{}:{:.3f}".format(x, float(fin[planned & (xcc == x)].max())) for x in xs))
    # how many waves of a SIMD are alive, as shares of the kernel, averaged over the SIMDs with `top` waves
    alive = np.zeros(top + 1)
    n_top = 0
    for idx in groups.values():
        if len(idx) != top:
            continue
        n_top += 1
        ends = np.sort(fin[idx])
        prev = 0.0
        for k, e in enumerate(ends):
            alive[top - k] += e - prev
            prev = e
        alive[0] += 1.0 - prev
    if n_top:
        show("  a SIMD with {} waves holds ".format(top) + ", ".join("{} alive for {:.3f}".format(k, alive[k] / n_top) for k in range(top, -1, -1)) +
             " of the kernel")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    if len(sys.argv) > 3:                         # a stamp file kept from an earlier run
        analyse(*read_stamps(sys.argv[3]))
        return
    path = os.environ.get("MP_UCT_WAVE_STAMPS") or os.path.join(tempfile.mkdtemp(), "uct_wave_stamps.bin")
    os.environ["MP_UCT_WAVE_STAMPS"] = path
    from rl_agents_amd import native
    from rl_agents_amd.envs import generators
    cfg = generators.highway_shaped(10, 10, 100, seed=0)
    ctx = native.Context(0)
    model = ctx.load_table(cfg["transition"], cfg["reward"], cfg["terminal"])
    non_term = np.flatnonzero(~cfg["terminal"])
    s0 = np.random.Generator(np.random.PCG64(12345)).choice(non_term, size=n).astype(np.int32)
    rng = np.random.Generator(np.random.PCG64(1)).integers(1, 2 ** 62, size=(n, 6)).astype(np.uint64)
    rng[:, 3] |= 1
    rng[:, 4:] = 0
    p = np.ones(5) / 5
    for _ in range(launches):
        ctx.uct_plan(model, s0, 33, 30, 0.8, 10.0, p, p, rng, max_plan_len=8)
    if not os.path.exists(path):
        sys.exit("no stamps were written: the library at {} was not built with -DMP_WAVE_STAMPS".format(native.lib_path()))
    print("{}: form {}, MP_UCT_BALANCE={}, launch {} of {}".format(native.lib_path(), ctx.last_kernel_variant(),
                                                                    os.environ.get("MP_UCT_BALANCE", "(unset)"), launches, launches))
    analyse(*read_stamps(path))
    ctx.close()


if __name__ == "__main__":
    main()
