#!/usr/bin/env python3
"""Selective unpack (capnp_gpu_unpack_batch_select) against the whole-batch
decode and against the gather workaround, on a config-2 store resident in
HBM: 1 Mi x 128-word chunks, 30 % zero words, packed with the record sync
index.

  a  the indexed decode of the whole store (unpack_batch_into, sync=...)
  b  select of every id in identity order
  c  select of a random permutation of every id
  d  select of 64 Ki random distinct ids
  e  the workaround for the ids of d: a torch gather of their packed bytes
     into a contiguous buffer, rebuilt offsets, unpack_batch_into without
     the index (the index is addressed by the store's word space and does
     not survive the gather).  Its buffer size is computed outside the
     timed region, so e pays no host synchronisation.
  B, D  b and d without the index (sync=None): the A/B of the indexed walk

Device events around each call, every leg warmed up, the legs alternated
within one process, medians over --reps repeats.  One JSON line on stdout
and in --out.

    python3 scripts/select_bench.py [--chunks N] [--sel K] [--reps R]
                                    [--legs abcdeBD] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "capnproto-rust_amd"))
sys.path.insert(0, ROOT)

CW = 128  # words per chunk (1 KiB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1 << 20)
    ap.add_argument("--sel", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="abcdeBD")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    from capnp_amd import Context, tile_chunks_for, unpack_tile_chunks_for
    assert torch.cuda.is_available(), "select_bench needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    n, k = args.chunks, min(args.sel, args.chunks)
    total = n * CW

    # the store
    offs = torch.arange(0, (n + 1) * CW, CW, dtype=torch.int64, device=dev)
    words = torch.empty(total, dtype=torch.int64, device=dev)
    ctx.gen_batch(words, offs, pz_thresh=bench.PZ["config2"])
    packed = torch.empty(ctx.batch_bound_bytes(total, n), dtype=torch.uint8, device=dev)
    poffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sync = torch.empty(ctx.sync_entries(total), dtype=torch.int32, device=dev)
    ctx.pack_batch_into(words, offs, packed, poffs, chunks_per_tile=tile_chunks_for(total, n),
                        sync=sync)
    torch.cuda.synchronize()
    packed_bytes = int(poffs[-1].item())

    g = torch.Generator(device="cpu").manual_seed(20)
    perm = torch.randperm(n, generator=g)
    ids_b = torch.arange(n, dtype=torch.int64, device=dev)
    ids_c = perm.to(dev)
    ids_d = perm[:k].clone().to(dev)
    ctx.reserve(n)  # (the select workspace covers every leg: no growth in the timed region)

    back = torch.empty(total, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    cons = torch.empty(n, dtype=torch.int64, device=dev)
    woff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    back_d = torch.empty(k * CW, dtype=torch.int64, device=dev)
    back_e = torch.empty(k * CW, dtype=torch.int64, device=dev)
    st_e = torch.empty(k, dtype=torch.int32, device=dev)
    utc_sync = unpack_tile_chunks_for(total, n, sync=True)
    utc_e = unpack_tile_chunks_for(k * CW, k)
    # e: what does not depend on the run (the gathered size: read once, outside the timing)
    e_bytes = int((poffs[ids_d + 1] - poffs[ids_d]).sum().item())
    ar_bytes = torch.arange(e_bytes, dtype=torch.int64, device=dev)
    zero1 = torch.zeros(1, dtype=torch.int64, device=dev)

    def leg_a():
        ctx.unpack_batch_into(packed, poffs, offs, back, st, cons, chunks_per_tile=utc_sync,
                              sync=sync)

    def select(ids, out, index=True):
        ctx.unpack_select_into(packed, poffs, offs, ids, out, woff[:ids.numel() + 1],
                               st[:ids.numel()], cons[:ids.numel()],
                               sync=sync if index else None)

    def leg_e():
        p0 = poffs[ids_d]
        lens = poffs[ids_d + 1] - p0
        noff = torch.cat([zero1, torch.cumsum(lens, 0)])
        src = torch.repeat_interleave(p0 - noff[:-1], lens, output_size=e_bytes) + ar_bytes
        buf = packed[src]
        wo = torch.cat([zero1, torch.cumsum(offs[ids_d + 1] - offs[ids_d], 0)])
        ctx.unpack_batch_into(buf, noff, wo, back_e, st_e, chunks_per_tile=utc_e)

    legs = {"a": (leg_a, total), "b": (lambda: select(ids_b, back), total),
            "c": (lambda: select(ids_c, back), total),
            "d": (lambda: select(ids_d, back_d), k * CW), "e": (leg_e, k * CW),
            "B": (lambda: select(ids_b, back, False), total),
            "D": (lambda: select(ids_d, back_d, False), k * CW)}
    legs = {x: legs[x] for x in args.legs}

    # every leg once, checked
    rows = words.view(n, CW)
    for name, (fn, _) in legs.items():
        back.zero_()
        fn()
        torch.cuda.synchronize()
        if name in "abB":
            assert torch.equal(back, words), name
        elif name == "c":
            assert torch.equal(back.view(n, CW), rows[ids_c]), name
        elif name in "dD":
            assert torch.equal(back_d.view(k, CW), rows[ids_d]), name
        else:
            assert torch.equal(back_e.view(k, CW), rows[ids_d]) and int(st_e.abs().sum()) == 0
        if name != "e":
            m = n if name not in "dD" else k
            assert int(st[:m].abs().sum()) == 0, name
    for _ in range(args.warmup):
        for fn, _ in legs.values():
            fn()
    torch.cuda.synchronize()

    s = torch.cuda.current_stream()
    ev = {x: [] for x in legs}
    for _ in range(args.reps):
        for name, (fn, _) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            ev[name].append((e0, e1))
    torch.cuda.synchronize()

    res = {"store": f"config2:{n}x{CW}", "packed_over_unpacked": round(packed_bytes / (8 * total), 4),
           "selected": k, "reps": args.reps, "legs": {}}
    for name, (_, nw) in legs.items():
        ms = sorted(a.elapsed_time(b) for a, b in ev[name])
        med = statistics.median(ms)
        res["legs"][name] = {"ms_median": round(med, 4), "ms_min": round(ms[0], 4),
                             "ms_max": round(ms[-1], 4), "words": nw,
                             "GiBps_unpacked": round(nw * 8 / med / 1e-3 / 2**30, 1)}
    if "a" in legs:
        pa = res["legs"]["a"]["ms_median"] / res["legs"]["a"]["words"]
        for name in "bcdBD":
            if name in legs:
                r = res["legs"][name]
                r["time_per_byte_over_a"] = round(r["ms_median"] / r["words"] / pa, 3)
    if "d" in legs and "e" in legs:
        res["d_over_e"] = round(res["legs"]["d"]["ms_median"] / res["legs"]["e"]["ms_median"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
