#!/usr/bin/env python3
"""Programs over more than 8 leaves under the f32-accumulating ops: a virtual
communicator's Allreduce and Reduce_scatter at p = 9 and 16 with MVX_SUM_ACC32
next to MPI_SUM on the same type, pair by pair.

Above 8 leaves MVX_SUM_ACC32 runs as several launches through f32 temporaries
(k_combine_f32 in and out, the MPI_FLOAT kernels in between; csrc/mvx_combine.c)
where MPI_SUM runs its own kernels on narrow temporaries, so the wide form
moves more bytes.  All ranks' buffers are on one GPU: the times are the whole
call (every rank's exchange copies and combines), HIP events on the stream.
`mis` shifts every send buffer by one element, which takes the narrow side of
the one-side-f32 launches off the word grid (their element path).

Prints one JSON line per config.
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES = ((72, "e4m3", 1), (65, "bf16", 2))


def run(mvx, comm, name, coll, p, n, dtype, e, op, shift, reps=5, warm=2):
    import torch
    sends = [torch.randint(0, 256, ((n + shift) * e + 64,), dtype=torch.uint8, device="cuda") for _ in range(p)]
    for s in sends:
        s.bitwise_and_(0x3f)          # small finite values: timing only
    ds = [s[shift * e:] for s in sends]
    if coll == "ar":
        recvs = [torch.empty(n * e, dtype=torch.uint8, device="cuda") for _ in range(p)]
    else:
        recvs = [torch.empty(n // p * e, dtype=torch.uint8, device="cuda") for _ in range(p)]

    def call():
        if coll == "ar":
            r, rcs = comm.allreduce_multi(ds, recvs, n, dtype, op)
        else:
            r, rcs = comm.reduce_scatter_multi(ds, recvs, [n // p] * p, dtype, op)
        assert r == 0 and rcs == [0] * p, (r, rcs)

    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"config": name, "coll": coll, "p": p, "elements_per_rank": n, "dtype": dtype, "op": op,
                      "shift_elements": shift, "last_kernel": mvx.last_kernel(),
                      "call_us": round(e0.elapsed_time(e1) * 1e3 / reps, 1)}), flush=True)


def main():
    mvx = importlib.import_module("mvapich-cce_amd")
    for p in (9, 16):
        comm = mvx.Comm.local_ranks(p, 0)
        try:
            n = (8 << 20) // p * p
            for dtype, tn, e in TYPES:
                for coll in ("ar", "rs"):
                    for shift, sn in ((0, "aligned"), (1, "mis")):
                        for op, on in ((mvx.MVX_SUM_ACC32, "acc32"), (mvx.MPI_SUM, "step")):
                            run(mvx, comm, "P%d-%s-%s-%s-%s" % (p, coll, tn, sn, on), coll, p, n, dtype, e, op, shift)
        finally:
            comm.free()


if __name__ == "__main__":
    main()
