"""NaN repair of one item's Sentinel inputs, the decision logic of ``Population_Dataset`` (data/PopulationDataset.py:419-441 weak-supervision
regions, :479-500 test windows) on device tensors; the fill itself is ``ops.nan_fill_`` (pc_nan_fill, csrc/nan_fill.hip).

  * S2 is filled whenever it holds a NaN (cloud-masked composites);
  * S1 (descending orbit) is filled when its NaN fraction is < 5 % and ``ascfill`` is off; otherwise the ascending orbit replaces it,
    which is filled when ITS fraction is < 5 % -- if not, the item raises the reference's ``Exception("No data here!")``.
    ``ascfill`` is a per-region setting of the reference (run_train.py:414, run_eval.py:227: ``need_asc = ["uga"]``).

The 5 % check needs the count on the host: ``fill_item_`` synchronises once per item (the count of the descending orbit; the reference
reads ``torch.isnan(S1).sum()`` there as well), and a second time when it falls back to the ascending orbit."""
from __future__ import annotations

import torch

MAX_NAN_FRACTION = 0.05


def nan_fraction_ok(nan_count, numel) -> bool:
    """``torch.isnan(S1).sum() / torch.numel(S1) < 0.05`` with the reference's own arithmetic (a float32 quotient)."""
    return bool(torch.tensor(int(nan_count)) / int(numel) < MAX_NAN_FRACTION)


def s1_orbit(nan_count, numel, ascfill):
    """The reference's choice for the descending S1 of an item with ``nan_count`` NaNs among ``numel`` entries: ("desc", fill?) keeps it
    (filled when it holds NaNs), ("asc", None) switches to the ascending orbit (whose own fraction then decides, ``asc_fill``)."""
    if nan_count == 0:
        return "desc", False
    if nan_fraction_ok(nan_count, numel) and not ascfill:
        return "desc", True
    return "asc", None


def asc_fill(nan_count, numel):
    """Whether the ascending S1 is filled (True), needs nothing (False); raises "No data here!" when it is too holey as well."""
    if nan_count == 0:
        return False
    if nan_fraction_ok(nan_count, numel):
        return True
    raise Exception("No data here!")


def _nan_count(t, count_only=True):
    from .. import ops
    return int(ops.nan_fill_(t, count_only=count_only).view(-1, 2)[:, 0].sum())


def fill_item_(s2, s1, load_s1_asc=None, ascfill=False):
    """Repair one item in place: ``s2`` (4, h, w) / ``s1`` (2, h, w) -- or (1, C, h, w) -- contiguous fp32 device tensors, either may be
    None.  ``load_s1_asc``: callable returning the ascending-orbit S1 of the same item (any device / dtype; copied into ``s1``).
    Returns the orbit of the S1 left in ``s1``: "desc", "asc", or None without S1."""
    from .. import ops
    if s2 is not None:
        ops.nan_fill_(s2)                          # a NaN-free S2 costs one read: every later launch returns at once
    if s1 is None:
        return None
    orbit, fill = s1_orbit(_nan_count(s1), s1.numel(), ascfill)
    if orbit == "desc":
        if fill:
            ops.nan_fill_(s1)
        return "desc"
    if load_s1_asc is None:
        raise ValueError("fill_item_: the descending S1 is too holey (or ascfill is set) and no ascending orbit was given")
    asc = load_s1_asc()
    s1.copy_(torch.as_tensor(asc).reshape(s1.shape))
    if asc_fill(_nan_count(s1), s1.numel()):
        ops.nan_fill_(s1)
    return "asc"


def select_s1_host(s1_desc, load_s1_asc, ascfill=False):
    """The same orbit choice for a HOST item (a dataset's ``__getitem__``; the fill itself runs later on the device, ``--nan_fill``):
    returns (S1 tensor of the chosen orbit, orbit name); raises "No data here!" like the reference."""
    orbit, _ = s1_orbit(int(torch.isnan(s1_desc).sum()), s1_desc.numel(), ascfill)
    if orbit == "desc":
        return s1_desc, "desc"
    asc = load_s1_asc()
    asc_fill(int(torch.isnan(asc).sum()), asc.numel())
    return asc, "asc"
