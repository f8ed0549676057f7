"""Fixture g13: the single-modality variants of g8 on the SHARED padded domain.

g8 (make_golden.py: g8_single_modality) is 48 x 40: add_padding gives 8 / 12 pixels there, the frozen building extractor pads 14, so the
two networks run on different domains.  At sides = 36 mod 64 both pad 14 and the fused training step runs them layer by layer in shared
launches, with the building score taken from the extractor's feature map on that domain.  36 x 36 is the smallest such size (pad 14 < 36:
the reflect rule holds; Hp = Wp = 64).  For a one-stream model the reference's score is the stream's own out conv (sar_out_conv /
optical_out_conv, networks.py:217-228), not a half of fusion_out_conv: this fixture pins it.

Keys: those of g8 under ``ic2/`` and ``ic4/``, plus the eval-mode dense outputs of ``model(sample, padding=False)`` under
``ic*/dense_pad0/`` (popdensemap, scale, building_counts).

Run from anywhere:  python tests/golden/make_golden_g13.py      (needs the reference checkout that make_golden.py names)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference, make_inputs, np_  # noqa: E402

NAME = "g13_single_modality_shared.npz"
HW = (36, 36)


def g13_single_modality_shared(popcorn, losses):
    out = {}
    for ic in (2, 4):
        torch.manual_seed(1600)
        m = popcorn.POPCORN(input_channels=ic, feature_extractor="DDA", occupancymodel=True, pretrained=True,
                            biasinit=0.9407, sentinelbuildings=True)
        m.train()
        for k, v in m.state_dict().items():
            if k.startswith("head."):
                out[f"ic{ic}/{k}"] = np_(v)
        x6, admin, census, y = make_inputs(90 + ic, 2, *HW)
        x = x6[:, :ic].contiguous()
        out[f"ic{ic}/input"], out[f"ic{ic}/admin_mask"], out[f"ic{ic}/census_idx"], out[f"ic{ic}/y"] = np_(x), np_(admin), np_(census), np_(y)
        torch.manual_seed(5)
        sample = {"input": x.clone(), "admin_mask": admin.clone(), "census_idx": census.clone(), "y": y.clone()}
        o = m(sample, train=True, padding=False, sparse=True)
        loss, _ = losses.get_loss(o, sample, scale=o["scale"], loss=["log_l1_loss"], lam=[1.0], scale_regularization=0.01, tag="weak")
        (loss * 100.0).backward()
        out[f"ic{ic}/popcount"], out[f"ic{ic}/popdensemap"], out[f"ic{ic}/scale"] = np_(o["popcount"]), np_(o["popdensemap"]), np_(o["scale"])
        out[f"ic{ic}/building_counts"] = np_(sample["building_counts"])
        out[f"ic{ic}/loss"] = np.float32(loss.item())
        gn = []
        for n, p in m.named_parameters():
            if p.grad is not None:
                gn.append(n)
                out[f"ic{ic}/grad/{n}"] = np_(p.grad)
        out[f"ic{ic}/grad_names"] = np.array(gn)
        with torch.no_grad():
            o2 = m({"input": x.clone()}, padding=True)
        out[f"ic{ic}/dense_pad1/popdensemap"] = np_(o2["popdensemap"])
        # eval mode, dense, padding=False: what validation and inference compute on this domain
        m.eval()
        with torch.no_grad():
            s3 = {"input": x.clone(), "admin_mask": admin.clone(), "census_idx": census.clone()}
            o3 = m(s3, padding=False)
        out[f"ic{ic}/dense_pad0/popdensemap"], out[f"ic{ic}/dense_pad0/scale"] = np_(o3["popdensemap"]), np_(o3["scale"])
        out[f"ic{ic}/dense_pad0/building_counts"] = np_(s3["building_counts"])
    return out


def main():
    popcorn, _, _, losses, _ = import_reference()
    out = g13_single_modality_shared(popcorn, losses)
    np.savez_compressed(os.path.join(OUT, NAME), **out)
    for ic in (2, 4):
        print(f"ic{ic}: loss {float(out[f'ic{ic}/loss']):.4f}  popcount {out[f'ic{ic}/popcount']}  grads {len(out[f'ic{ic}/grad_names'])}  "
              f"nonzero density px {int((out[f'ic{ic}/popdensemap'] != 0).sum())}")


if __name__ == "__main__":
    main()
