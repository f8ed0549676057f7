"""The expected batch of a resident atlas, built on the host: every crop is cut out of its OWN region by tests/region_oracle.py's item
builder, then the items are padded to the batch maximum by the existing collate -- what the reference's ConcatDataset of per-country
datasets and its collate produce (run_train.py:423-431).  Also the three test regions of tests/test_gpu_atlas.py."""
import torch

from tests import region_oracle as R

REFERENCE_BANDS = (2, 1, 0, 3, 0, 1)
MODEL_ORDER_BANDS = (0, 1, 2, 3, 0, 1)
# (h, w), seasons, S2 bands, S1 bands, band selection: a wrong region's stride, extent, band map or season count shows up
SPECS = [((37, 53), 1, 4, 2, REFERENCE_BANDS), ((64, 48), 2, 5, 3, MODEL_ORDER_BANDS), ((96, 128), 2, 6, 2, MODEL_ORDER_BANDS)]
PAYLOADS = (0x7FC12345, -0x3FFFFF, 0x7FC00777)                      # quiet NaNs with payloads (never the poison's all-ones)


def make_region(k, kind="f32", layer=False, asc=False):
    """Host tensors of test region k: values distinct per (region, season, band, pixel) -- S2 = a counter below 60000 (exact in uint16 and
    fp32), S1 = another counter as fp32 --, NaNs with payloads in S1 (and in fp32 S2), an irregular boundary of 9 units."""
    (h, w), S, C2, C1, bands = SPECS[k]
    n2, n1 = S * C2 * h * w, S * C1 * h * w
    s2 = ((torch.arange(n2, dtype=torch.int64) * 7 + 1000 * k + 13) % 59999).reshape(S, C2, h, w)
    s2 = s2.to(torch.uint16) if kind == "u16" else s2.float()
    s1 = (-(torch.arange(n1, dtype=torch.float32) * 0.25) - 100.0 * (k + 1)).reshape(S, C1, h, w).contiguous()
    s1.view(torch.int32)[0, 1, 3:9, 4:40] = PAYLOADS[0]
    s1.view(torch.int32)[S - 1, 0, h - 7:h, w - 7:w] = PAYLOADS[1]
    if kind == "f32":
        s2.view(torch.int32)[S - 1, bands[3], h - 12:h - 2, 0:33] = PAYLOADS[2]
    out = {"s2": s2, "s1": s1, "boundary": R.irregular_raster(h, w, units=9, seed=2 + k), "band_sel": bands,
           "census_idx": torch.arange(1, 10), "census_pop": torch.rand(9, generator=torch.Generator().manual_seed(3 + k)) * 2000 + 1}
    if asc:
        out["s1_asc"] = (s1.nan_to_num(0.0) * 0.5 - 7.0).contiguous()
    if layer:
        b = (torch.arange(h * w, dtype=torch.float32) * 0.125 + k).reshape(h, w).contiguous()
        b.view(torch.int32)[h // 2, 1:w - 1] = PAYLOADS[0]
        out["buildings"] = b
    return out


def atlas_items(regions, region_of, crops, orbit=None):
    """One host item per crop, from its own region (orbit[b] == 1: the region's ascending S1)."""
    items = []
    for b, (k, c) in enumerate(zip(region_of, crops)):
        r = regions[int(k)]
        s1 = r["s1_asc"] if orbit is not None and int(orbit[b]) else r["s1"]
        it = R.weaksup_item(r["s2"], s1, r["boundary"], r["band_sel"], c[:4], int(c[4]), 0.0, 0, (0, 0, 0, 0))
        if r.get("buildings") is not None:
            x0, x1, y0, y1 = (int(v) for v in c[:4])
            it["building_counts"] = r["buildings"][x0:x1, y0:y1][None].clone()
        items.append(it)
    return items


def host_atlas_batch(regions, region_of, crops, orbit=None, hw=None):
    """{"S2", "S1", "admin_mask", "data_hw"[, "building_counts"]} as the host collate pads them (0 / 0 / -1 / 0.0); hw: a larger tile."""
    out = R.host_batch(atlas_items(regions, region_of, crops, orbit), multi=False)
    if hw is not None:
        Hm, Wm = out["admin_mask"].shape[-2:]
        pad = (0, hw[1] - Wm, 0, hw[0] - Hm)
        for key, fill in (("S2", 0.0), ("S1", 0.0), ("admin_mask", -1.0), ("building_counts", 0.0)):
            if key in out:
                out[key] = torch.nn.functional.pad(out[key], pad, value=fill)
    return out
