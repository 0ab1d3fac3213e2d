"""Driver of tests/test_gpu_setop_multi_lb_retry.py: the fused set-op kernel (setop_multi_tile_kernel) through the look-back
watchdog's retry, run once in THIS process against the library UKM_LIB_PATH names.  Not collected by pytest; started as
`python tests/setop_multi_lb_driver.py OUT.jsonl`.  Harness, data and the meaning of the marks: tests/lb_retry_driver.py.

One case: union + inter + diff of two sets of 16,000 codes, 32,000 merged records = 3.3 tiles of 9728.  Under the seam
library every tile >= 1 of the first launch gives its look-back up at once -- match prefix 0: inter written at 0, diff at
a_t, the union at d_t + s_t --, the host repeats the launch with ticketed tile ids and the context stays on tickets.
"""
import json
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import lb_retry_driver as D  # noqa: E402

UID = (D.OP_UNION, D.OP_INTER, D.OP_DIFF)
NAME = "setop2_multi-uid-small"
MARKS = [list(m) for m in D.STANDARD]      # a fresh context, the call, the same call again


def run(h):
    A, B = D.sets(D.SMALL)
    want = {op: D.oracle_fn(h.O, op)([A, B]) for op in UID}
    dA, dB = h.up(A, D.U64), h.up(B, D.U64)
    for what in ("first call", "repeated call"):
        got = h.ctx.setop2_multi(dA, dB, ops=UID, out={op: h.out(D.U64, len(want[op])) for op in UID})
        for op in UID:
            h.same(got[op], want[op], "%s, op %d" % (what, op))
        h.mark()
        h.check_guards()
    h.check_inputs()
    assert h.ctx.stat("setop_multi_fused") == 2 and h.ctx.stat("setop_multi_split") == 0


def main(out_path):
    h = D.H()
    rec = {"name": NAME, "error": None}
    t0 = time.time()
    status = 0
    try:
        h.begin()
        run(h)
        h.end()
    except Exception as e:
        rec["error"] = traceback.format_exc()
        # a HIP error may be a GPU fault: the process ends here either way
        if (isinstance(e, h.L.UkmError) and e.code == h.L.ERR_HIP) or "HIP error" in str(e) or "hipError" in str(e):
            status = 3
    rec["wd"] = h.wd
    rec["seconds"] = round(time.time() - t0, 3)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(rec) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
