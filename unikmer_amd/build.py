"""Builds libunikmer_hip.so (gfx950) in-tree with hipcc, and the test library libunikmer_hip_lbtest.so beside it.
`python -m unikmer_amd.build`."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libunikmer_hip.so")
SOURCES = ["ukm_ctx.hip", "ukm_setops.hip", "ukm_scan.hip", "ukm_sort.hip", "ukm_encode.hip",
           "ukm_tax.hip", "ukm_nway.hip", "ukm_kway.hip", "ukm_comm.hip", "ukm_fold.hip", "ukm_probe.hip", "ukm_probe_union.hip", "ukm_probe_ranked.hip", "ukm_place.hip", "ukm_pfold.hip", "ukm_srmerge.hip", "ukm_route.hip", "ukm_map.hip", "ukm_select.hip", "ukm_tsplit.hip", "ukm_unik.hip", "ukm_text.hip", "ukm_deflate.hip", "ukm_inflate.hip", "ukm_fastx.hip", "ukm_pairs.hip", "ukm_screen.hip"]
HEADERS = ["ukm_internal.h", "ukm_device.h", "ukm_kway.h", "ukm_fold.h", "ukm_probe.h", "ukm_pfold.h", "ukm_srmerge.h", "ukm_route.h", "ukm_map.h", "ukm_dir.h", "ukm_bytes.h", "ukm_huff.h", "ukm_inflate.h", "ukm_setop_part.h", "ukm_setop_tile.h", "ukm_setop_kernels.h", "ukm_setop_order.h", "ukm_win_common.h", "ukm_win_kernels.h", "ukm_win_minimizer.h", "ukm_pairs.h", "ukm_screen.h", "ukm_sort_state.h", "ukm_sort_plan.h", "ukm_sort_kernels.h", "ukm_sort_buckets.h", os.path.join("..", "..", "include", "unikmer_hip.h")]
# The test library (tests/test_gpu_lb_retry.py): the sources that include the decoupled look-back, compiled once more with
# the watchdog's injection seam of ukm_device.h (UKM_LB_TEST_TIMEOUT) into objects of their own, and linked with the product
# objects of all other sources.  The product library never sees the macro.
SO_LBTEST = os.path.join(HERE, "libunikmer_hip_lbtest.so")
LBTEST_SOURCES = ["ukm_setops.hip", "ukm_scan.hip", "ukm_encode.hip", "ukm_select.hip", "ukm_tsplit.hip", "ukm_map.hip"]
LBTEST_FLAG = "-DUKM_LB_TEST_TIMEOUT"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    objs_lbtest = []
    procs = []
    jobs = [(src, src.replace(".hip", ".o"), []) for src in SOURCES]
    jobs += [(src, src.replace(".hip", "_lbtest.o"), [LBTEST_FLAG]) for src in LBTEST_SOURCES]
    for src, obj, extra in jobs:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, obj)
        if not extra:
            objs.append(o)
            if src not in LBTEST_SOURCES:
                objs_lbtest.append(o)
        else:
            objs_lbtest.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = [_hipcc()] + FLAGS + extra + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            procs.append((src, o, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for src, o, p in procs:
        out, _ = p.communicate()
        text = out.decode(errors="replace")
        if p.returncode != 0:
            failed = True
            sys.stderr.write("hipcc failed for %s:\n%s\n" % (src, text))
        elif "reserved registers" in text or "failed to meet occupancy target" in text:
            # ukm_sort_kernels.h's hand-scheduled match_any8 (compiled into ukm_sort.hip) names s80..s83 in its clobber list: if a change of register
            # budget ever makes the compiler reserve them (or miss a declared occupancy) the build must not go on
            failed = True
            first = [ln for ln in text.splitlines() if "reserved registers" in ln or "occupancy target" in ln][:3]
            sys.stderr.write("register-budget check failed for %s:\n%s\n" % (src, "\n".join(first)))
            try:
                os.remove(o)
            except OSError:
                pass
        elif verbose and out:
            sys.stderr.write(text)
    if failed:
        raise RuntimeError("building libunikmer_hip.so failed")
    if force or procs or _stale(SO, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    if force or procs or _stale(SO_LBTEST, objs_lbtest):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO_LBTEST] + objs_lbtest + ["-ldl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    build_cli(force=force, verbose=verbose)
    return SO


HOST = os.path.join(HERE, "host")
CLI = os.path.join(HERE, "bin", "unikmer")


def build_cli(force=False, verbose=False):
    """the `unikmer`-compatible C++ driver (host side of the drop-in), linked against the C ABI"""
    # one translation unit, main.cpp, that includes the other files of host/: every one of them is a dependency
    srcs = [os.path.join(HOST, f) for f in sorted(os.listdir(HOST))] + [os.path.join(HERE, "..", "include", "unikmer_hip.h")]
    if not (force or _stale(CLI, srcs + [SO])):
        return CLI
    os.makedirs(os.path.dirname(CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", os.path.join(HOST, "main.cpp"), "-o", CLI,
           "-L" + HERE, "-lunikmer_hip", "-lz", "-pthread", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return CLI


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
