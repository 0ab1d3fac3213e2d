#!/usr/bin/env python3
"""ukm_fastx: the device's FASTA/Q parser on three shapes of text, and `unikmer count` end to end with the parser on the
device, on the host, and in the parent commit's driver.

    python tools/fastx_bench.py [--mbp 100] [--steps 7] [--warmup 2] [--e2e-runs 5] [--parent-bin PATH/unikmer]
                                [--tmp DIR] [--out profiles/fastx.json]

Texts: the bases of tests/golden/*.fasta.gz, repeated to about --mbp million bases, as (1) FASTA in 60-column lines under the
genomes' own headers, (2) FASTA with every record on one line, (3) four-line FASTQ of 150-base reads.  Per text, on device
tensors and into outputs of the exact size: ukm_fastx with LAST, timed with the context's own event timer (ukm_last_call_ms),
median of --steps calls behind --warmup calls, with the smallest and the largest; GB/s of text; the split of the call -- the
size side (a size query's ukm_last_call_ms), of which its scan step (ukm_last_kernel_ms), and the write side (the rest) --; a
device-to-device copy of the text's bytes timed in the same run.  The results are compared with tests/fastx_model.py on the
first 4 MB of each text.

End to end: `unikmer count -k 31 -K -s` on text (1), uncompressed and gzipped, wall time of --e2e-runs runs behind one that
is not counted: this build with UNIKMER_DEVICE_FASTX=1 and with UNIKMER_HOST_FASTX=1, and --parent-bin (the parent commit's
driver) when given, both ways as well (a parent from before the switch takes the host parser either way); the outputs must be
the same bytes.
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SWITCHES = ("UNIKMER_DEVICE_FASTX", "UNIKMER_HOST_FASTX", "UNIKMER_FASTX_REPORT", "UNIKMER_CHUNK_MB")


def file_digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def genomes():
    """(header line, bases) of every record of the golden genomes"""
    out = []
    for f in sorted(os.listdir(GOLDEN)):
        if not f.endswith(".fasta.gz"):
            continue
        with gzip.open(os.path.join(GOLDEN, f), "rb") as fh:
            for rec in fh.read().split(b">")[1:]:
                name, _, body = rec.partition(b"\n")
                out.append((b">" + name.rstrip(b"\r"), body.replace(b"\n", b"").replace(b"\r", b"")))
    return out


def wrap(seq, width):
    a = np.frombuffer(seq, dtype=np.uint8)
    full = len(a) // width * width
    lines = np.empty((full // width, width + 1), dtype=np.uint8)
    lines[:, :width] = a[:full].reshape(-1, width)
    lines[:, width] = 10
    return lines.tobytes() + (a[full:].tobytes() + b"\n" if full < len(a) else b"")


def texts(mbp):
    recs = genomes()
    per = sum(len(s) for _, s in recs)
    reps = max(1, round(mbp * 1e6 / per))
    fa60, fa1, fq = [], [], []
    for r in range(reps):
        for name, s in recs:
            nm = name + b" copy %d" % r
            fa60.append(nm + b"\n" + wrap(s, 60))
            fa1.append(nm + b"\n" + s + b"\n")
            a = np.frombuffer(s, dtype=np.uint8)
            n = len(a) // 150
            g = np.empty((n, 16 + 1 + 150 + 3 + 150 + 1), dtype=np.uint8)
            ids = np.char.zfill(np.arange(n).astype("S14"), 14)
            g[:, 0] = ord("@")
            g[:, 1] = ord("r")
            g[:, 2:16] = np.frombuffer(ids.tobytes(), dtype=np.uint8).reshape(n, 14)
            g[:, 16] = 10
            g[:, 17:167] = a[: n * 150].reshape(n, 150)
            g[:, 167:170] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            g[:, 170:320] = ord("I")
            g[:, 320] = 10
            fq.append(g.tobytes())
    return {"FASTA, 60-column lines": (b"".join(fa60), False), "FASTA, one line per record": (b"".join(fa1), False),
            "FASTQ, four lines, 150-base reads": (b"".join(fq), True)}, per * reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=100)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastx.json"))
    a = ap.parse_args()
    assert a.steps >= 5 and a.e2e_runs >= 5

    import torch
    from unikmer_amd import lib
    import fastx_model as M
    if not torch.cuda.is_available():
        raise SystemExit("fastx_bench.py needs the GPU")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    tmp = tempfile.mkdtemp(prefix="fastx_bench_", dir=a.tmp)
    tx, n_bases = texts(a.mbp)

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ts = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    rows = []
    for name, (text, fastq) in ({} if a.no_kernels else tx).items():
        head = text[: 4 << 20]
        wb, wr, wh, wc, ws = M.device(head, fastq, False)
        hb, hr, hh, hc, hs = ctx.fastx(torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).to(dev), fastq=fastq, last=False)
        assert (hc, hs) == (wc, ws) and hb.cpu().numpy().tobytes() == wb and hr.cpu().numpy().view(np.uint64).tolist() == [int(x) for x in wr] \
            and hh.cpu().numpy().view(np.uint64).tolist() == [int(x) for x in wh], "the device's result is not the model's: " + name
        t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
        b, r, h, consumed, stop = ctx.fastx(t, fastq=fastq, last=True)
        assert consumed == len(text) and stop == lib.FASTX_STOP_NONE
        out = (torch.empty(b.numel(), dtype=torch.uint8, device=dev), torch.empty(r.numel(), dtype=torch.int64, device=dev),
               torch.empty(max(h.numel(), 1), dtype=torch.int64, device=dev)[: h.numel()])
        nb, nr = b.numel(), h.numel()
        del b, r, h
        call, scan, query = [], [], []
        for i in range(a.warmup + a.steps):
            ctx.fastx(t, fastq=fastq, last=True, out=out)
            t_call, t_scan = ctx.last_call_ms(), ctx.last_kernel_ms()
            try:
                ctx.fastx(t, fastq=fastq, last=True, out=(out[0][:0], out[1][:1], out[2][:0]))    # capacities 0: ends behind the size side
                raise AssertionError("a size query of a text with records must fail for capacity")
            except lib.CapacityError as e:
                assert e.needed == (nb, nr)
            t_query = ctx.last_call_ms()
            if i >= a.warmup:
                call.append(t_call)
                scan.append(t_scan)
                query.append(t_query)
        ms, qms, sms = statistics.median(call), statistics.median(query), statistics.median(scan)
        cms = copy_ms(len(text))
        row = {"text": name, "text_bytes": len(text), "bases": nb, "records": nr,
               "call_ms": ms, "call_ms_min": min(call), "call_ms_max": max(call), "GBps_text": len(text) / ms / 1e6,
               "GBps_text_min": len(text) / max(call) / 1e6, "GBps_text_max": len(text) / min(call) / 1e6,
               "size_side_ms": qms, "scan_step_ms": sms, "write_side_ms": ms - qms,
               "copy_ms": cms, "copy_GBps": len(text) / cms / 1e6, "frac_of_copy": cms / ms}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del t, out
        torch.cuda.empty_cache()

    e2e = []
    plain = os.path.join(tmp, "in.fa")
    with open(plain, "wb") as fh:
        fh.write(tx["FASTA, 60-column lines"][0])
    gz = os.path.join(tmp, "in.fa.gz")
    with gzip.open(gz, "wb", compresslevel=6) as fh:
        fh.write(tx["FASTA, 60-column lines"][0])
    del tx
    ctx.trim()
    for path, kind in ((plain, "uncompressed"), (gz, "gzip")):
        sums = {}
        for label, exe, env in (("device_fastx", BIN, {"UNIKMER_DEVICE_FASTX": "1"}), ("host_fastx", BIN, {"UNIKMER_HOST_FASTX": "1"}),
                                ("parent_device_fastx", a.parent_bin, {"UNIKMER_DEVICE_FASTX": "1"}),
                                ("parent_host_fastx", a.parent_bin, {"UNIKMER_HOST_FASTX": "1"})):
            if exe is None:
                continue
            env_all = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            env_all.update(env)
            out = os.path.join(tmp, "out_" + label)
            ts = []
            for i in range(a.e2e_runs + 1):
                t0 = time.perf_counter()
                subprocess.check_call([exe, "count", "-k", "31", "-K", "-s", path, "-o", out], env=env_all, stderr=subprocess.DEVNULL)
                if i:
                    ts.append(time.perf_counter() - t0)
                    print("# %s %s: %.3f s" % (kind, label, ts[-1]), flush=True)
            sums[label] = file_digest(out + ".unik")
            e2e.append({"command": "count -k 31 -K -s in.fa%s -o out" % (".gz" if kind == "gzip" else ""), "input": kind, "input_bytes": os.path.getsize(path),
                        "bases": n_bases, "binary": label, "out_file_bytes": os.path.getsize(out + ".unik"),
                        "wall_s_median": statistics.median(ts), "wall_s_min": min(ts), "wall_s_max": max(ts), "wall_s": ts})
            print(json.dumps(e2e[-1]), flush=True)
            os.remove(out + ".unik")
        assert len(set(sums.values())) == 1, "the outputs differ: %r" % sums

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    doc = {"tool": "tools/fastx_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "e2e_runs": a.e2e_runs, "rows": rows, "end_to_end": e2e}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    shutil.rmtree(tmp, ignore_errors=True)
    ctx.close()


if __name__ == "__main__":
    main()
