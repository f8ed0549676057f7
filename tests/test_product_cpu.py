"""Product grid, the parts that need no GPU: the two run_eval flags, the cell-grid geometry helper, and the float64 yardstick of
tests/test_gpu_product.py against a brute-force per-cell loop (the yardstick itself must not be wrong)."""
import torch


def test_eval_parser_product_flags():
    from popcorn_amd.cli import eval_parser
    a = eval_parser().parse_args([])
    assert a.product_cell == 0 and a.product_out is None
    a = eval_parser().parse_args("--product_cell 10 --product_out p.pt".split())
    assert a.product_cell == 10 and a.product_out == "p.pt"


def test_product_shape():
    from popcorn_amd.eval import product_shape
    assert product_shape(150, 170, 10) == (15, 17)
    assert product_shape(151, 169, 10) == (16, 17)
    assert product_shape(23, 31, 1) == (23, 31)
    assert product_shape(23, 31, 64) == (1, 1)
    assert product_shape(2304, 2560, 10) == (231, 256)


def test_reference_equals_brute_force_per_cell_loop():
    from popcorn_amd.eval import get_patch_indices
    from tests.test_gpu_product import product_reference
    h, w, ps, ov, M, cell = 23, 31, 12, 2, 3, 5
    g = torch.Generator().manual_seed(1)
    wins = [(x, y, torch.rand(M, ps, ps, generator=g)) for x, y, s in get_patch_indices(h, w, ps, ov, True).tolist()]
    planes, mean, std, visits = product_reference(h, w, wins, ps, ov, cell)
    hc, wc = -(-h // cell), -(-w // cell)
    assert planes.shape == (M, hc, wc) and planes.dtype == torch.float64
    inside = lambda x, y, r, c: x + ov <= r < x + ps - ov and y + ov <= c < y + ps - ov  # noqa: E731
    want = torch.zeros(M, hc, wc, dtype=torch.float64)
    for r in range(h):
        for c in range(w):
            hits = [(x, y, pd) for x, y, pd in wins if inside(x, y, r, c)]
            assert int(visits[r, c]) == len(hits)
            for x, y, pd in hits:
                want[:, r // cell, c // cell] += pd[:, r - x, c - y].double() / len(hits)
    assert int(visits.max()) == 16 and int(visits.min()) == 0
    torch.testing.assert_close(planes, want, rtol=1e-13, atol=0)
    for i in range(hc):
        for j in range(wc):
            t = want[:, i, j]
            m = sum(t.tolist()) / M
            assert abs(float(mean[i, j]) - m) <= 1e-13 * max(m, 1e-300)
            s = (sum((v - m) ** 2 for v in t.tolist()) / (M - 1)) ** 0.5
            assert abs(float(std[i, j]) - s) <= 1e-9 * max(m, 1e-300)
