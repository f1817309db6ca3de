#!/usr/bin/env python3
"""Host issue cost of a device-buffer call: an 8-byte MPI_Allreduce (MPI_SUM on
two MPI_FLOAT) on a virtual 2-rank communicator through api.py -- the eager
path mvxi_run_device -> mvxi_run_device_eager -> mvxi_exec_group.  Prints one
JSON line: the median and the quartiles of the per-call host time.

  issue_cost.py [--lib PATH/libmvx.so] [--calls N] [--warmup W] [--tag NAME]

--lib loads another build of the host library (an A/B against this tree's)."""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import torch
    mvx = importlib.import_module("mvapich-cce_amd")
    if a.lib:
        mvx.LIB_COLL = os.path.abspath(a.lib)
    p, n = 2, 2
    comm = mvx.Comm.local_ranks(p, 0)
    send = [torch.full((n,), float(r + 1), device="cuda:0") for r in range(p)]
    recv = [torch.zeros(n, device="cuda:0") for _ in range(p)]
    st = torch.cuda.current_stream().cuda_stream
    us = []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter_ns()
        r, rcs = comm.allreduce_multi(send, recv, n, mvx.MPI_FLOAT, mvx.MPI_SUM, st)
        t1 = time.perf_counter_ns()
        assert r == 0 and rcs == [0] * p, (r, rcs)
        if i >= a.warmup:
            us.append((t1 - t0) / 1e3)
    torch.cuda.synchronize()
    assert all(x.tolist() == [3.0] * n for x in recv), [x.tolist() for x in recv]
    comm.free()
    us.sort()
    with open("/proc/self/maps") as f:          # the host library this process really mapped
        libs = sorted({ln.split()[-1] for ln in f if ln.rstrip().endswith("/libmvx.so")})
    print(json.dumps({"probe": "8-byte Allreduce, 2 virtual ranks, api.py", "tag": a.tag,
                      "lib": libs, "calls": a.calls,
                      "median_us": round(us[len(us) // 2], 3), "q1_us": round(us[len(us) // 4], 3),
                      "q3_us": round(us[3 * len(us) // 4], 3)}))


if __name__ == "__main__":
    main()
