"""Launch trace of the per-launch engine: every call that engine.py / train.py / the model make into ``popcorn_amd.ops`` (module
functions and ``WgradBatch`` methods), one JSON line per call, one file per case -- to diff two checkouts of the engine:

    POPCORN_NATIVE_STEP=0 python tools/engine_trace.py OUT_DIR [case-name substring]     (same file, PYTHONPATH = either checkout)

A tensor is rendered as (token, shape, strides, dtype), token = index of first appearance of its data_ptr() in the case; a PcBn as the
index of first appearance of its id.  Every rendered object stays referenced until the case ends, so no address is reused.  The
``*_ok`` geometry predicates enqueue nothing and are not recorded (which launch follows them is).  Needs a GPU; a case is one step.

The cases: the fused step at the three geometries (same padded domain for both networks, separate domains with B = 2 and B = 1), in both
precisions, the three truncation regimes, every engine switch, the three input forms, single modality, a given building layer; the same
step with multi-unit supervision (2-D ``census_idx``, K = 3 with one padded slot and one absent unit: ``units-*``), also on a given building
layer and on the split form; the model API (autograd and eval) and the engine called directly.
"""
import inspect
import json
import os
import sys

os.environ["POPCORN_NATIVE_STEP"] = "0"
sys.path.insert(0, os.getcwd())
import torch                                                         # noqa: E402
from popcorn_amd import _lib as L, engine as E, ops, train as T      # noqa: E402
from popcorn_amd.data import stats                                   # noqa: E402
from popcorn_amd.data.synthetic import make_raw_batch                # noqa: E402
from popcorn_amd.model import POPCORN                                # noqa: E402

LINES, SEEN, KEEP, DEPTH = [], {}, [], [0]


def token(kind, key, obj):
    KEEP.append(obj)
    return SEEN.setdefault((kind, key), len(SEEN))


def render(v):
    if torch.is_tensor(v):
        return ["T", token("t", v.data_ptr(), v), list(v.shape), list(v.stride()), str(v.dtype)]
    if type(v).__name__ == "PcBn":
        return ["bn", token("bn", id(v), v)]
    if isinstance(v, dict):
        return {str(k): render(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [render(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (torch.device, torch.dtype)):
        return str(v)
    return v.item() if hasattr(v, "item") else ["obj", type(v).__name__, token("o", id(v), v)]


def wrap(owner, name, label):
    fn = getattr(owner, name)
    sig = inspect.signature(fn)

    def traced(*a, **kw):
        if DEPTH[0] == 0:          # (calls that ops makes into itself belong to the call that made them)
            bound = sig.bind(*a, **kw)          # positional or by keyword, defaults spelled out or not: the same call
            bound.apply_defaults()
            LINES.append(json.dumps([label, render(dict(bound.arguments))], sort_keys=True))
        DEPTH[0] += 1
        try:
            return fn(*a, **kw)
        finally:
            DEPTH[0] -= 1
    setattr(owner, name, traced)


for n_, f_ in list(vars(ops).items()):
    if inspect.isfunction(f_) and f_.__module__ == ops.__name__ and not n_.startswith("_") and not n_.endswith("_ok"):
        wrap(ops, n_, n_)
for n_, f_ in list(vars(ops.WgradBatch).items()):
    if inspect.isfunction(f_) and (not n_.startswith("_") or n_ == "__init__"):
        wrap(ops.WgradBatch, n_, "WgradBatch." + n_)

SHAPES = [(2, 100, 100), (2, 64, 48), (1, 150, 90)]
REGIMES = {"full": {}, "enc": {"encoder_no_grad": True}, "unet": {"unet_no_grad": True}}
OFF = lambda *names: {n: False for n in names}  # noqa: E731
SWITCHES = {"fp32": [{}, OFF("COMPOSED_UP"), OFF("FUSED_LEVEL2"), OFF("FUSED_LEVEL2_BWD"), OFF("FUSED_CONV_BWD"), OFF("PADDED_INPUT"),
                     OFF("COMPOSED_UP", "FUSED_LEVEL2", "FUSED_LEVEL2_BWD", "PADDED_INPUT", "FUSED_CONV_BWD"), {"conv_split": 0}],
            "bf16": [{}, OFF("FUSED_CONV_BWD"), OFF("FUSED_LEVEL2"), OFF("FUSED_LEVEL2_BWD"), OFF("FUSED_UPT"), OFF("PADDED_INPUT")]}


def model(prec="fp32", ic=6, senb=True):
    torch.manual_seed(1600)
    return POPCORN(ic, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=senb).cuda().set_precision(prec)


def sample(B, H, W, form="input", ic=6, units=False):
    b = make_raw_batch(B, H, W, seed=H * 1000 + W, device="cuda", region="disc")
    s = {k: b[k] for k in ("admin_mask", "census_idx", "y")}
    if units:
        # multi-unit supervision: per crop the ring, the disc and a unit that is not in it; the first row's last slot is padding
        ids = b["census_idx"]
        s["census_idx"] = torch.stack([ids + B, ids, torch.full_like(ids, 999)], 1)
        s["census_idx"][0, 2] = -1
        s["census_n"] = [2] + [3] * (B - 1)
        s["y"] = torch.rand(B, 3, generator=torch.Generator().manual_seed(5)).cuda() * 500.0
    sel = b["raw"][:, list(stats.BAND6)]
    if form == "raw":
        s["raw"] = b["raw"]
    elif form == "split":
        s["raw_s2"] = sel[:, :4].round().clamp(0, 65535).to(torch.int32).cpu().to(torch.uint16).cuda().contiguous()
        s["raw_s1"] = sel[:, 4:6].contiguous()
    else:
        x = ops.select_normalize(b["raw"], stats.BAND6, stats.MEAN6, stats.STD6)
        s["input"] = {6: x, 2: x[:, 4:6].contiguous(), 4: x[:, :4].contiguous()}[ic]
    return s


def step(prec, B, H, W, form="input", ic=6, senb=True, units=False, **regime):
    s = sample(B, H, W, form, ic, units)
    if not senb:
        s["building_counts"] = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    tr = T.FusedTrainStep(model(prec, ic, senb), lr=1e-4, weight_decay=1e-5, gradient_clip=0.01)
    return lambda: tr.step(s, **regime)


def api_train(prec, B, H, W, padding, **regime):
    m, s = model(prec).train(), sample(B, H, W)
    return lambda: m(s, train=True, padding=padding, sparse=True, **regime)["popcount"].sum().backward()


def api_eval(B, H, W):
    m, x = model().eval(), torch.randn(B, 6, H, W, generator=torch.Generator().manual_seed(H * 300 + W)).cuda()

    def run():
        with torch.no_grad():
            m({"input": x}, padding=True)
    return run


def engine_pass(prec, B, H, W, **kw):
    """UNetEngine.forward + backward on the 14-pixel padded domain, called directly (on this thread: autograd runs the model API's
    backward on its own, where the standard ``trace`` module does not count lines)"""
    m = model(prec)
    eng, x = m.engines()[0], sample(B, H, W)["input"]
    grads = {n: torch.zeros_like(p) for n, p in zip(*m.trainable())}

    def run():
        with L.precision(prec):
            feats, saved = eng.forward(x, 14, 14, H + 28, W + 28, save=True)
            eng.backward(saved, L.as_act(torch.ones_like(feats, dtype=torch.float32)), grads, prefix="unetmodel.", **kw)
    return run


def cases():
    for prec, switches in SWITCHES.items():
        for sw in switches:
            for rname, regime in REGIMES.items():
                for shp in SHAPES:
                    yield f"{prec}-{'+'.join(sw) or 'defaults'}-{rname}-{'x'.join(map(str, shp))}", sw, (lambda: step(prec, *shp, **regime))
        for form in ("raw", "split"):           # ("input" is the form of the cases above)
            for rname, regime in REGIMES.items():
                for shp in SHAPES:
                    yield f"{prec}-{form}-{rname}-{'x'.join(map(str, shp))}", {}, (lambda: step(prec, *shp, form=form, **regime))
        # the model API: autograd path on the 128^2 domain and on odd padded sizes (pooling on the fly, Up blocks with a zero frame)
        for rname, regime in list(REGIMES.items())[:2]:
            yield f"{prec}-api-{rname}-2x100x100", {}, (lambda: api_train(prec, 2, 100, 100, False, **regime))
            yield f"{prec}-api-padded-{rname}-1x77x59", {}, (lambda: api_train(prec, 1, 77, 59, True, **regime))
            yield f"{prec}-engine-padded-{rname}-1x77x59", {}, (lambda: engine_pass(prec, 1, 77, 59, **regime))
        yield f"{prec}-engine-accumulate-2x100x100", {}, (lambda: engine_pass(prec, 2, 100, 100, accumulate=True))
        yield f"{prec}-given-buildings", {}, (lambda: step(prec, 2, 100, 100, senb=False))
        for rname, regime in REGIMES.items():
            for shp in SHAPES:
                yield f"{prec}-units-{rname}-{'x'.join(map(str, shp))}", {}, (lambda: step(prec, *shp, units=True, **regime))
        for shp in SHAPES[:2]:
            yield f"{prec}-units-given-buildings-{'x'.join(map(str, shp))}", {}, (lambda: step(prec, *shp, senb=False, units=True))
        yield f"{prec}-units-split", {}, (lambda: step(prec, 2, 100, 100, form="split", units=True))
    for ic in (2, 4):           # one stream; 64 x 48: the extractor runs on its own domain (UNetEngine.building_score)
        for shp in SHAPES[:2]:
            yield f"fp32-single-modality-{ic}-{'x'.join(map(str, shp))}", {}, (lambda: step("fp32", *shp, ic=ic))
    yield "fp32-no-deferred-head-reduce", {"DEFER_HEAD_REDUCE": False}, (lambda: step("fp32", 2, 100, 100))
    yield "fp32-eval-1x100x100", {}, (lambda: api_eval(1, 100, 100))
    yield "fp32-eval-1x82x117", {}, (lambda: api_eval(1, 82, 117))      # tests/test_gpu_fuzz.py: padded width 145, reflect loaders
    yield "fp32-eval-1x40x1100", {}, (lambda: api_eval(1, 40, 1100))    # wider than the shared padded input takes
    yield "fp32-eval-1x100x102", {}, (lambda: api_eval(1, 100, 102))    # exact halving, rows not 16-byte aligned: the composed Up declines


def main(out, only=""):
    os.makedirs(out, exist_ok=True)
    total = 0
    for name, sw, make in cases():
        if only not in name:
            continue
        prev = {k: getattr(T if hasattr(T, k) else E, k) for k in sw if k != "conv_split"}
        split = L.lib().pc_set_conv_split(sw["conv_split"]) if "conv_split" in sw else None
        for k in prev:
            setattr(T if hasattr(T, k) else E, k, sw[k])
        try:
            run = make()
            del LINES[:], KEEP[:]
            SEEN.clear()
            try:
                run()
            except (ValueError, AssertionError, NotImplementedError, L.PopcornHipError) as e:      # a rejected input is behaviour too
                LINES.append(json.dumps(["raised", type(e).__name__, str(e)]))
            torch.cuda.synchronize()
        finally:
            for k, v in prev.items():
                setattr(T if hasattr(T, k) else E, k, v)
            if split is not None:
                L.lib().pc_set_conv_split(split)
        with open(os.path.join(out, name + ".jsonl"), "w") as f:
            f.write("\n".join(LINES) + "\n")
        total += len(LINES)
        print(f"{name}: {len(LINES)} calls", flush=True)
    print(f"total: {total} calls")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
