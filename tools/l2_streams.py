#!/usr/bin/env python3
"""tools/l2_streams.py [--out PREFIX] [--timeout S]  ->  PREFIX_tcc.txt, PREFIX_tcp.txt

L2 and L1 counters per kernel launch of one C3 frame, in the format of profiles/r03a_pmc_tcc.txt (one line per launch, in
launch order).  Two rocprofv3 --pmc passes over `python bench.py --child-frames 3`, each a run of its own with nothing but the
kernel trace beside the counters:

    pass tcc   TCC_HIT_sum TCC_MISS_sum
    pass tcp   TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum

Each pass runs under a time limit in a process group of its own, which is killed as a whole when the limit runs out (as
bench.py's run_counter_passes does).  The launches written are those of the LAST of the three frames; the profiler serialises
kernels, so the traversal launches do not see the shading launches that run beside them in a timed frame.  The summary at the
end gives, per traversal launch, the L2 hit rate, and the frame's sums.  FOVPT_SO selects the library, as everywhere."""
import argparse
import csv
import glob
import os
import re
import shutil
import signal
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = {
    "tcc": ["TCC_HIT_sum", "TCC_MISS_sum"],
    "tcp": ["TCP_TCC_READ_REQ_sum", "TCP_TOTAL_CACHE_ACCESSES_sum"],
}


def run_pass(exe, counters, timeout_s):
    """-> the dispatches of the run in launch order: [{"k": kernel, "dur_us": .., counter: value, ..}], or raises RuntimeError"""
    d = tempfile.mkdtemp(prefix="fovpt_l2s_", dir=os.environ.get("TMPDIR", "/tmp"))
    cmd = [exe, "--pmc"] + counters + ["--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--",
                                       sys.executable, os.path.join(ROOT, "bench.py"), "--child-frames", "3"]
    try:
        proc = subprocess.Popen(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            _, err = proc.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            for sig in (signal.SIGTERM, signal.SIGKILL):
                try:
                    os.killpg(proc.pid, sig)                    # the group this function started, nothing else
                except ProcessLookupError:
                    break
                try:
                    proc.communicate(timeout=10)
                    break
                except subprocess.TimeoutExpired:
                    continue
            raise RuntimeError("timed out after %d s (its process group was killed)" % timeout_s)
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if proc.returncode != 0 or not files:
            raise RuntimeError("no counters (rc %d): %s" % (proc.returncode, (err or "").strip()[-400:]))
        disp = {}
        for f in files:
            for row in csv.DictReader(open(f)):
                m = re.search(r"\b(k_[a-z_0-9]+)(?:<[^>]*>)?\s*\(", row["Kernel_Name"])
                if not m:
                    continue
                dd = disp.setdefault(int(row["Dispatch_Id"]), {"k": m.group(1)})
                dd[row["Counter_Name"]] = dd.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
                if row.get("Start_Timestamp") and row.get("End_Timestamp"):
                    dd["dur_us"] = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        return [disp[i] for i in sorted(disp)]
    finally:
        shutil.rmtree(d, ignore_errors=True)


def last_frame(dispatches):
    """the launches from the last k_generate / k_generate_owned on, up to and including the k_resolve that ends its frame"""
    starts = [i for i, dd in enumerate(dispatches) if dd["k"].startswith("k_generate")]
    if not starts:
        return dispatches
    frame = dispatches[starts[-1]:]
    ends = [i for i, dd in enumerate(frame) if dd["k"] == "k_resolve"]
    return frame[:ends[-1] + 1] if ends else frame


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="l2_streams", help="prefix of the two files written")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per pass")
    args = ap.parse_args()
    exe = shutil.which("rocprofv3")
    if not exe:
        sys.exit("rocprofv3 not on PATH")
    for tag, counters in PASSES.items():
        try:
            frame = last_frame(run_pass(exe, counters, args.timeout))
        except RuntimeError as e:
            sys.exit("pass %s: %s" % (tag, e))                  # nothing more is started on the GPU after a pass that failed
        path = "%s_%s.txt" % (args.out, tag)
        with open(path, "w") as f:
            for dd in frame:
                f.write("%s dur_us=%d %s\n" % (dd["k"], round(dd.get("dur_us", 0)), " ".join("%s=%d" % (c, dd.get(c, 0)) for c in counters)))
        print("%s: %d launches" % (path, len(frame)))
        a, b = counters
        tot = [0.0, 0.0]
        for dd in frame:
            tot[0] += dd.get(a, 0)
            tot[1] += dd.get(b, 0)
            if dd["k"] == "k_traverse":
                if tag == "tcc":
                    print("  k_traverse %4d us  hit %9d  miss %9d  L2 hit rate %5.1f %%" % (dd.get("dur_us", 0), dd.get(a, 0), dd.get(b, 0),
                                                                                            100.0 * dd.get(a, 0) / max(1.0, dd.get(a, 0) + dd.get(b, 0))))
                else:
                    print("  k_traverse %4d us  L1 -> L2 reads %9d  L1 accesses %9d  (%5.1f %% go to L2)" % (dd.get("dur_us", 0), dd.get(a, 0), dd.get(b, 0),
                                                                                                            100.0 * dd.get(a, 0) / max(1.0, dd.get(b, 0))))
        print("  frame: %s %d  %s %d" % (a, tot[0], b, tot[1]))


if __name__ == "__main__":
    main()
