#!/usr/bin/env python3
"""Timing of K4's inverse on the GPU: reef_decompress host to host and its kernel alone (HIP events), the windowed square root
against the Tonelli-Shanks form of the same kernel in the same job, and reef_hyrax_eval_comm_compressed against reef_hyrax_eval_comm.
    python tools/time_decompress.py [profiles/r08_decompress_timing.txt]
Host-to-host figures are of the release build.  The kernel-alone figures and the comparison of the two roots need the switches of
the +experiment build (REEF_DECOMPRESS_EVENTS, REEF_DECOMPRESS_ROOT): the same sources, the same kernels."""
import ctypes
import os
import re
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reef_amd import _ffi, msm                       # noqa: E402
from reef_amd.hyrax import HyraxEval                 # noqa: E402

RUNS = 5
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def stat(ms):
    """median and spread (max - min) of the runs"""
    return statistics.median(ms), max(ms) - min(ms)


def fmt(ms):
    med, spread = stat(ms)
    return f"{med:9.3f} ms  spread {spread:6.3f}  ({' '.join('%.3f' % v for v in ms)})"


def encodings(curve, n, k0=77):
    """n points (GPU-generated) and their encodings through reef_normalize"""
    aff = msm.gen_bases(curve, k0, 3, n)
    base = msm.PALLAS_BASE_P if msm.curve_id(curve) == 0 else msm.PALLAS_SCALAR_Q
    jac = np.zeros((n, 12), dtype=np.uint64)
    jac[:, :8] = aff
    jac[:, 8:] = msm.scalar_to_limbs((1 << 256) % base)
    return aff, msm.normalize(curve, jac, affine=False, compressed=True)[1]


def kernel_ms(exp, cid, d_in, n, d_out, root):
    """one reef_decompress of the +experiment build on device buffers with the kernel bracketed by events: (kernel ms, call ms)"""
    if root == "tonelli_shanks":
        os.environ["REEF_DECOMPRESS_ROOT"] = "0"
    else:
        os.environ.pop("REEF_DECOMPRESS_ROOT", None)
    bad = ctypes.c_uint64(0)
    t = time.perf_counter()
    st = exp.reef_decompress(cid, d_in.ptr, n, _ffi.REEF_DEVICE, d_out.ptr, ctypes.byref(bad), None)
    call = (time.perf_counter() - t) * 1e3
    assert st == 0 and bad.value == 0, exp.reef_last_error()
    m = re.search(rb"kernel ([0-9.]+) us", exp.reef_last_error())
    assert m, "the +experiment build did not report the kernel's time"
    return float(m.group(1)) / 1e3, call


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r08_decompress_timing.txt")
    lib, exp = _ffi.load(), _ffi.load_experiment()
    assert lib.reef_device_count() > 0, "no GPU: nothing here is measured without one"
    say(f"# tools/time_decompress.py: {RUNS} runs each, median, spread = max - min; library sources {_ffi.library_sources_sha16()}")
    say(f"# {lib.reef_version().decode()} / {exp.reef_version().decode()}")
    say()
    say("## reef_decompress: host encodings -> host affine points (release build), and the kernel alone (HIP events, +experiment build, device buffers)")
    os.environ["REEF_DECOMPRESS_EVENTS"] = "1"
    at_8192 = {}
    for curve in ("pallas", "vesta"):
        cid = msm.curve_id(curve)
        for logn in (10, 12, 13, 14):
            n = 1 << logn
            aff, comp = encodings(curve, n)
            got, bad, _ = msm.decompress(curve, comp)                     # warm, and the result is the points
            assert bad == 0 and (got == aff).all()
            h2h = []
            for _ in range(RUNS):
                t = time.perf_counter()
                msm.decompress(curve, comp, out=got)
                h2h.append((time.perf_counter() - t) * 1e3)
            d_in, d_out = msm.DeviceBuffer.from_host(comp), msm.DeviceBuffer(64 * n)
            outs, ker = {}, {"windowed": [], "tonelli_shanks": []}
            for root in ker:                                                # warm both code paths, and both give the same bytes
                kernel_ms(exp, cid, d_in, n, d_out, root)
                outs[root] = d_out.to_host((n, 8)).tobytes()
            assert outs["windowed"] == outs["tonelli_shanks"] == aff.tobytes()
            for _ in range(RUNS):                                           # alternating, in one job
                for root in ker:
                    ker[root].append(kernel_ms(exp, cid, d_in, n, d_out, root)[0])
            say(f"{curve:6s} n = 2^{logn:<2d} host to host        {fmt(h2h)}")
            say(f"{curve:6s} n = 2^{logn:<2d} kernel windowed     {fmt(ker['windowed'])}")
            say(f"{curve:6s} n = 2^{logn:<2d} kernel Tonelli-Sh.  {fmt(ker['tonelli_shanks'])}")
            if logn == 13:
                at_8192[curve] = ker
    os.environ.pop("REEF_DECOMPRESS_ROOT", None)
    os.environ.pop("REEF_DECOMPRESS_EVENTS", None)
    say()
    say("## which root ships: the windowed one iff it is faster at n = 2^13 by more than the run-to-run spread of five runs each")
    for curve, ker in at_8192.items():
        (mw, sw), (mt, st) = stat(ker["windowed"]), stat(ker["tonelli_shanks"])
        verdict = "windowed" if mt - mw > max(sw, st) else "tonelli_shanks"
        say(f"{curve:6s} windowed {mw:.3f} ms (spread {sw:.3f}), Tonelli-Shanks {mt:.3f} ms (spread {st:.3f}), ratio {mt / mw:.2f}: {verdict}")
    say()
    say("## reef_hyrax_eval_comm_compressed against reef_hyrax_eval_comm (the parent's path: affine host rows), two row sets in turn so every call re-keys")
    for curve in ("pallas", "vesta"):
        for left in (12, 13):
            rows, num_vars = 1 << left, left + 1
            sets = [encodings(curve, rows, k0) for k0 in (5, 9)]
            z = np.arange(1 << num_vars, dtype=np.uint64).astype(np.uint8)
            point = [3 + 7 * i for i in range(num_vars)]
            with msm.MsmContext(curve, msm.gen_bases(curve, 1, 1, 2), bucket_groups=4) as key, HyraxEval(curve, z, num_vars, left) as hx:
                hx.eval_begin(key, point)
                want = [hx.eval_comm(a).tobytes() for a, _ in sets]
                assert [msm.compress(curve, hx.eval_comm_compressed(c)) for _, c in sets] == [msm.compress(curve, np.frombuffer(w, np.uint64)) for w in want]
                t_aff, t_cmp, t_same_aff, t_same_cmp = [], [], [], []
                for i in range(2 * RUNS):                                   # alternating forms and row sets
                    a, c = sets[i % 2]
                    t = time.perf_counter()
                    hx.eval_comm(a)
                    t_aff.append((time.perf_counter() - t) * 1e3)
                    t = time.perf_counter()
                    hx.eval_comm_compressed(c)
                    t_cmp.append((time.perf_counter() - t) * 1e3)
                for i in range(RUNS):                                       # the same host bytes again: no decode, no re-key
                    hx.eval_comm(sets[0][0])
                    t = time.perf_counter()
                    hx.eval_comm(sets[0][0])
                    t_same_aff.append((time.perf_counter() - t) * 1e3)
                    hx.eval_comm_compressed(sets[0][1])
                    t = time.perf_counter()
                    hx.eval_comm_compressed(sets[0][1])
                    t_same_cmp.append((time.perf_counter() - t) * 1e3)
            t_aff, t_cmp = t_aff[::2][:RUNS], t_cmp[::2][:RUNS]             # five runs of each, on row set 0
            say(f"{curve:6s} 2^{left} rows eval_comm (affine)        {fmt(t_aff)}")
            say(f"{curve:6s} 2^{left} rows eval_comm_compressed      {fmt(t_cmp)}")
            say(f"{curve:6s} 2^{left} rows increment                 {stat(t_cmp)[0] - stat(t_aff)[0]:9.3f} ms")
            say(f"{curve:6s} 2^{left} rows same bytes again, affine  {fmt(t_same_aff)}")
            say(f"{curve:6s} 2^{left} rows same bytes again, compr.  {fmt(t_same_cmp)}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
