"""Torch restatement of the device-N unit layout's contract (pc_unit_layout_dev, include/popcorn_hip.h), on the CPU: what every element of
every capacity-sized output holds for given (census_idx, y, counts as they stand in device memory).  Shared by the CPU and the GPU tests."""
import torch

I64_MAX = torch.iinfo(torch.int64).max


def layout_dev_ref(census_idx, y, counts):
    """census_idx (B, K) int64, y (B, K) fp32, counts: B integers, ANY value (clamped into [1, K] like the kernel does).  Returns a dict
    of CPU tensors: units int64 [B K] (tail INT64_MAX), unit_off int32 [B + 1], y_sorted fp32 [B K] (tail 0), dest int32 [B K] (tail -1),
    N, Ncap.  Ties among equal ids keep the caller's order (the kernel's (id, slot) total order)."""
    B, K = census_idx.shape
    Ncap = B * K
    cn = [min(max(int(c), 1), K) for c in counts]
    units = torch.full((Ncap,), I64_MAX, dtype=torch.int64)
    y_sorted = torch.zeros(Ncap, dtype=torch.float32)
    dest = torch.full((Ncap,), -1, dtype=torch.int32)
    off = [0]
    for b, c in enumerate(cn):
        ids = census_idx[b, :c].tolist()
        order = sorted(range(c), key=lambda k: (ids[k], k))
        for j, src in enumerate(order):
            n = off[-1] + j
            units[n] = ids[src]
            y_sorted[n] = y[b, src]
            dest[n] = off[-1] + src
        off.append(off[-1] + c)
    return {"units": units, "unit_off": torch.tensor(off, dtype=torch.int32), "y_sorted": y_sorted, "dest": dest, "N": off[-1],
            "Ncap": Ncap, "counts": cn}
