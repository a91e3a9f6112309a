"""Bit-level comparison of two LIBRARIES on the rig-refinement trial kernels (csrc/mvmc_rigfit.hip), under this tree's Python (GPU):
    python tools/rig_kernel_diff.py LIB_A.so LIB_B.so [--json OUT.json]
For a change of the kernels that must not change a number: LIB_A is a build of the parent's csrc (from a ``git worktree``), LIB_B this
tree's build.  Each library runs in a fresh child process (MVMC_LIB_PATH) at kernel level, with the packing helpers of the tests:
  * every case of tests/rig_cases.py through mvmc_rig_accumulate / mvmc_rig_step at variant 1 and variant 0, and through the _robust
    entries with loss none, Huber and Cauchy; every (case, loss) of tests/rig_robust_cases.py through the _robust entries;
  * every case of tests/rig_intr_cases.py through the _intr entries;
  * the several-sequences-in-one-launch packings of test_gpu_rig_kernels.py, test_gpu_rig_robust.py and test_gpu_rig_intr.py;
each after the first trial and after the whole solve.  Compared with np.array_equal(..., equal_nan=True): X, X_trial, cams,
cams_trial, info, ctl, red, part2 and, where the helper returns them, mvmc_rig_weights' w.  (part is scratch: not compared.)  Exit
status 1 when anything differs."""
import json, os, subprocess, sys, tempfile
import numpy as np

ARRAYS = ("X", "X_trial", "cams", "cams_trial", "info", "ctl", "red", "part2", "w")


def child(path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import rig_cases as rc
    import rig_intr_cases as rci
    import rig_refine_np as rr
    import rig_robust_cases as rcs
    import test_gpu_rig_intr as ti
    import test_gpu_rig_robust as tr
    out = {}

    def keep(tag, res):
        for k in ARRAYS:
            if k in res:
                out[f"{tag}:{k}"] = res[k]

    def both(tag, solve):
        """after the first trial and after the whole solve"""
        keep(tag + "/first", solve(steps=1))
        keep(tag + "/whole", solve())

    for name in rc.CASES:
        c, p = rc.case(name), rc.params(name)
        for variant in (1, 0):
            both(f"plain/{name}/variant{variant}", lambda **kw: tr.device_solve([c["prob"]], c["K"], [c["Rt"]], plain=True, variant=variant, **p, **kw))
        for loss in (None, "huber", "cauchy"):
            both(f"robust/{name}/{loss}", lambda **kw: tr.device_solve([c["prob"]], c["K"], [c["Rt"]], loss=loss, **p, **kw))
    for name, loss in tr.PAIRS:
        c, p = rcs.case(name), rcs.params(name)
        both(f"robust_cases/{name}/{loss}", lambda **kw: tr.device_solve([c["prob"]], c["K"], [c["Rt"]], loss=loss, **p, **kw))
    for name in rci.CASES:
        c, p = rci.case(name), rci.params(name)
        both(f"intr/{name}", lambda **kw: ti.device_solve([c["prob"]], [c["K"]], [c["Rt"]], **p, **kw))
    # several sequences in one launch, as the three test files pack them
    names = ["reject", "stopped", "c5_65", "bad", "xtol"]
    cs = [rc.case("c5_65" if n == "stopped" else n) for n in names]
    stop0 = [tr.STOP_FEW_CAMERAS if n == "stopped" else 0 for n in names]
    both("several/plain", lambda **kw: tr.device_solve([c["prob"] for c in cs], cs[0]["K"], [c["Rt"] for c in cs], plain=True, stop0=stop0,
                                                       max_iter=8, mu0=1e-6, ftol=rr.LM_FTOL, xtol=1e-3, **kw))
    for loss in rcs.LOSSES:
        for names, p in ((["reject", "stopped", "c5_65", "xtol", "delta_small"], dict(max_iter=8, mu0=1e-4, ftol=1e-12, xtol=rcs.params("xtol")["xtol"])),
                         (["c8", "c8_b"], dict(max_iter=5, mu0=1e-3, ftol=1e-12, xtol=1e-10))):
            cs = [rcs.case({"stopped": "c5_65", "c8_b": "c8"}.get(n, n)) for n in names]
            Rts = [c["Rt"] if n != "c8_b" else rr.perturb_rig(c["Rt_true"], 99) for n, c in zip(names, cs)]
            stop0 = [tr.STOP_FEW_CAMERAS if n == "stopped" else 0 for n in names]
            both(f"several/robust/{loss}/{names[0]}", lambda **kw: tr.device_solve([c["prob"] for c in cs], cs[0]["K"], Rts, loss=loss, stop0=stop0,
                                                                                   **p, **kw))
    names = ["reject", "stopped", "f_c5_65", "xtol", "tight"]
    cs = [rci.case({"stopped": "f_c5_65"}.get(n, n)) for n in names]
    stop0 = [ti.STOP_FEW_CAMERAS if n == "stopped" else 0 for n in names]
    for mode in (dict(intrinsics="focal", focal_sigma=0.05), dict(intrinsics="focal+centre", focal_sigma=0.05, centre_sigma_px=10.0)):
        both(f"several/intr/{mode['intrinsics']}", lambda **kw: ti.device_solve(
            [c["prob"] for c in cs], [c["K"] for c in cs], [c["Rt"] for c in cs], stop0=stop0, max_iter=6, mu0=1e-4, ftol=1e-12,
            xtol=rci.params("xtol")["xtol"], **mode, **kw))
    print(f"{os.environ['MVMC_LIB_PATH']}: {len(out)} arrays")
    np.savez(path, **out)


def main():
    args = sys.argv[1:]
    out_json = None
    if "--json" in args:
        k = args.index("--json")
        out_json = args[k + 1]
        del args[k:k + 2]
    res = []
    for lib in (os.path.abspath(p) for p in args[:2]):
        f = tempfile.mktemp(suffix=".npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f], env=dict(os.environ, MVMC_LIB_PATH=lib), check=True, timeout=300)
        res.append(dict(np.load(f)))
        os.remove(f)
    x, y = res
    bad = sorted(set(x) ^ set(y)) + [k for k in sorted(set(x) & set(y)) if not (x[k].dtype == y[k].dtype and np.array_equal(
        x[k], y[k], equal_nan=x[k].dtype.kind == "f"))]
    groups = sorted({k.split("/")[0] + ("/" + k.split("/")[1] if k.startswith("several") else "") for k in x})
    record = dict(compared=list(ARRAYS), after=["the first trial", "the whole solve"], groups={}, arrays=len(x),
                  values=int(sum(v.size for v in x.values())), differences=len(bad), differing=bad[:50])
    for g in groups:
        ks = [k for k in x if k.startswith(g + "/")]
        n_bad = sum(k in bad for k in ks)
        record["groups"][g] = dict(runs=len({k.split(":")[0] for k in ks}), arrays=len(ks), differences=n_bad)
        print(f"{g:24s} {len(ks):6d} arrays  {sum(x[k].size for k in ks):9d} values  " + ("bit-identical" if not n_bad else f"{n_bad} DIFFER"))
    for k in bad[:20]:
        print("differs:", k)
    print("ALL BIT-IDENTICAL" if not bad else f"{len(bad)} arrays differ")
    if out_json:
        with open(out_json, "w") as fh:
            json.dump(record, fh, indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main())
