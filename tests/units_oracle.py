"""Plain-torch restatement of multi-unit census supervision (one crop, K census units, one pass), and the replicated batch it is defined by.

The definition: a batch (input[B], admin_mask[B], census_idx[B, K], y[B, K]) gives what the reference gives for the N = sum K_b samples
(input[b], admin_mask[b], census_idx[b, k], y[b, k]) with the same two multinomial draws.  ``replicate`` builds that batch for the committed
oracle (oracle/popcorn_oracle.py, untouched: it is the yardstick); ``units_forward`` is the one-pass form -- union mask, per-unit sums --
built from the oracle's own network pieces.  The per-pixel helpers (``unit_slots``, ``unit_mask``, ``unit_sums``, ``unit_paint``) are
what the HIP kernels of csrc/units.hip are tested against."""
import torch

from oracle import popcorn_oracle as O


def counts_of(census_idx, census_n=None):
    B, K = census_idx.shape
    return [K] * B if census_n is None else [int(c) for c in census_n]


def replicate(inputs, y=None):
    """The replicated one-unit batch of a multi-unit batch: (inputs', y_flat), replicas in (b, k) order over the valid slots."""
    cn = counts_of(inputs["census_idx"], inputs.get("census_n"))
    rows = [b for b, c in enumerate(cn) for _ in range(c)]
    out = {"input": inputs["input"][rows], "admin_mask": inputs["admin_mask"][rows],
           "census_idx": torch.stack([inputs["census_idx"][b, k] for b, c in enumerate(cn) for k in range(c)])}
    if "building_counts" in inputs:
        out["building_counts"] = inputs["building_counts"][rows]
    y_flat = None if y is None else torch.stack([y[b, k] for b, c in enumerate(cn) for k in range(c)])
    return out, y_flat, rows


def unit_slots(admin_mask, census_idx, census_n=None):
    """slot (B, H, W) int64: the flat (b, k) index -- the caller's order -- of the listed unit that owns the pixel, else -1.  The id compare
    is the reference's ``admin_mask == census_idx`` (float ids)."""
    cn = counts_of(census_idx, census_n)
    slot = torch.full(admin_mask.shape, -1, dtype=torch.int64)
    n = 0
    for b, c in enumerate(cn):
        for k in range(c):
            slot[b][admin_mask[b] == census_idx[b, k].to(admin_mask.dtype)] = n
            n += 1
    return slot, n


def sorted_order(census_idx, census_n=None):
    """to_caller (N,): the flat index, in the per-sample ASCENDING order of the ids the kernels work in, of caller slot n."""
    cn = counts_of(census_idx, census_n)
    out, off = [], 0
    for b, c in enumerate(cn):
        rank = torch.argsort(torch.argsort(census_idx[b, :c]))
        out.append(off + rank)
        off += c
    return torch.cat(out)


def unit_mask(building, slot, rowsel, colsel, occupancymodel=True):
    """get_sparsity_mask (popcorn.py:361-377) with region := slot >= 0, the selection grid given as row / column flags.
    Returns (mask bool (B, H, W), nsel, nregion) after the batch-wide empty-selection fallback (:374-375)."""
    reg = slot >= 0
    mask = (building[:, 0] > 0) & reg if occupancymodel else reg.clone()
    mask = mask | (rowsel.bool()[None, :, None] & colsel.bool()[None, None, :])
    mask = mask & reg
    if mask.sum() == 0:
        mask = reg
    return mask, int(mask.sum()), int(reg.sum())


def draw_selection(H, W):
    """The two CPU-generator draws of get_sparsity_mask (popcorn.py:366-369) as row / column flags."""
    sub = 60
    xi = torch.ones(H).multinomial(num_samples=min(sub, H), replacement=False)
    yi = torch.ones(W).multinomial(num_samples=min(sub, W), replacement=False)
    rs, cs = torch.zeros(H, dtype=torch.uint8), torch.zeros(W, dtype=torch.uint8)
    rs[xi] = 1
    cs[yi] = 1
    return rs, cs


def unit_sums(popdense, slot, N, dtype=torch.float64):
    """popcount[n] = sum of popdense over slot == n, accumulated in ``dtype``."""
    out = torch.zeros(N, dtype=dtype)
    ok = slot >= 0
    out.index_add_(0, slot[ok], popdense[ok].to(dtype))
    return out


def unit_paint(g_popcount, slot):
    out = torch.zeros(slot.shape, dtype=g_popcount.dtype)
    ok = slot >= 0
    out[ok] = g_popcount[slot[ok]]
    return out


def units_forward(sd, inputs, padding=True, sparse=False, occupancymodel=True, sentinelbuildings=True):
    """POPCORN.forward for a 2-D census_idx in one pass (cf. O.popcorn_forward): popcount (N,) in (b, k) order, popdensemap (B, H, W),
    scale = scale[mask] in (b, y, x) order of the union mask (sparse) or the map."""
    X = inputs["input"]
    S1, S2 = {6: (True, True), 2: (True, False), 4: (False, True)}[X.shape[1]]
    if "building_counts" not in inputs or sentinelbuildings:
        inputs["building_counts"] = O.create_building_score(sd, X, S1, S2)
    slot, N = unit_slots(inputs["admin_mask"], inputs["census_idx"], inputs.get("census_n"))
    mask = None
    if sparse:
        rs, cs = draw_selection(X.shape[2], X.shape[3])
        mask, _, _ = unit_mask(inputs["building_counts"], slot, rs, cs, occupancymodel)
    Xp, pads = O.add_padding(X, padding)
    feats = O.dualstream_features(sd, "unetmodel", O.reorder_channels(Xp, S1, S2), False, S1, S2)
    headin = O.revert_padding(feats, pads)
    out = O.sparse_head_forward(sd, headin, mask)[:, 0] if sparse else O.head_forward(sd, headin)[:, 0]
    res = {"mask": mask, "slot": slot}
    if occupancymodel:
        scale = O.ForceDecisions.out_relu(out, mask if sparse else None)
        res["scale"] = scale[mask] if sparse else scale
        popdensemap = scale * inputs["building_counts"][:, 0]
    else:
        popdensemap = O.ForceDecisions.out_relu(out, mask if sparse else None)
        res["scale"] = None
    # per-unit sums, each like the reference's (popdensemap * region).sum((1, 2)) of its replica
    res["popcount"] = torch.stack([(popdensemap * (slot == n)).sum() for n in range(N)])
    res["popdensemap"] = popdensemap
    return res


def units_train_step_grads(sd, inputs, y, lam_weak=100.0, scale_regularization=0.01, loss=("log_l1_loss",), lam=(1.0,), occupancymodel=True):
    """forward(padding=False, sparse=True) -> get_loss over the N pairs -> (loss * lam_weak).backward(), cf. O.train_step_grads."""
    names = O.trainable_names(sd)
    work = dict(sd)
    for n in names:
        work[n] = sd[n].detach().clone().requires_grad_(True)
    out = units_forward(work, inputs, padding=False, sparse=True, occupancymodel=occupancymodel)
    _, y_flat, _ = replicate(inputs, y)
    l, _ = O.get_loss(out, {"y": y_flat}, scale=out["scale"], loss=loss, lam=lam, scale_regularization=scale_regularization, tag="weak")
    (l * lam_weak).backward()
    grads = {n: work[n].grad for n in names if work[n].grad is not None}
    return l.detach(), {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, grads


def replicated_train_step_grads(sd, inputs, y, lam_weak=100.0, scale_regularization=0.01, loss=("log_l1_loss",), lam=(1.0,),
                                occupancymodel=True):
    """The committed oracle on the replicated batch (O.train_step_grads restated only to pass ``occupancymodel`` through)."""
    rep, y_flat, _ = replicate(inputs, y)
    names = O.trainable_names(sd)
    work = dict(sd)
    for n in names:
        work[n] = sd[n].detach().clone().requires_grad_(True)
    out = O.popcorn_forward(work, rep, padding=False, sparse=True, occupancymodel=occupancymodel)
    l, _ = O.get_loss(out, {"y": y_flat}, scale=out["scale"], loss=loss, lam=lam, scale_regularization=scale_regularization, tag="weak")
    (l * lam_weak).backward()
    grads = {n: work[n].grad for n in names if work[n].grad is not None}
    return l.detach(), {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, grads


def make_case(B=2, H=96, W=80, units=((3, 7, 12), (5, 9)), channels=6, seed=11, pad_to=None):
    """A multi-unit batch on vertical-band tilings: sample b is cut into len(units[b]) + 2 irregular bands -- the listed units next to two
    unlisted neighbours (ids 40 + b, 50 + b) -- with a -1 frame on the right / bottom edge like the collate's padding.  Returns
    (inputs, y): census_idx (B, K) padded with -1, census_n, y (B, K)."""
    g = torch.Generator().manual_seed(seed)
    K = max(len(u) for u in units) if pad_to is None else pad_to
    X = torch.randn(B, channels, H, W, generator=g)
    admin = torch.full((B, H, W), -1.0)
    cidx = torch.full((B, K), -1, dtype=torch.int64)
    y = torch.zeros(B, K)
    xx = torch.arange(W - 5).float()[None, :]
    yy = torch.arange(H - 3).float()[:, None]
    for b in range(B):
        ids = [40 + b] + list(units[b]) + [50 + b]
        nb = len(ids)
        band = ((xx + 6.0 * torch.sin(yy / 9.0 + b)) * nb / (W - 5)).floor().clamp(0, nb - 1).long()      # wavy bands
        admin[b, :H - 3, :W - 5] = torch.tensor(ids, dtype=torch.float32)[band]
        cidx[b, :len(units[b])] = torch.tensor(units[b])
        y[b, :len(units[b])] = torch.rand(len(units[b]), generator=g) * 300.0
    return {"input": X, "admin_mask": admin, "census_idx": cidx, "census_n": [len(u) for u in units]}, y
