"""Records tests/golden/posembed_*.npz from the REFERENCE's own classes, in float32 on the CPU: PositionEmbeddingSine and
PositionEmbeddingSineWithLearnableTemporal (src/models/position_encoding.py) and DeformableTransformer.prepare_data with
get_valid_ratio (src/models/deformable_transformer.py), called unbound on a stand-in that has the level embedding (the whole
transformer needs the attention extension).  Tensors only; each file under 32 KiB.

    python tests/golden/make_golden_posembed.py /path/to/reference

The reference modules are imported as make_golden_labelloss.py imports them -- a package whose __init__ is skipped, with
stand-ins for what the imports pull in and never call here.

Cases: the 2D sine encoding of a 5 x 7 mask with a rectangular padding and holes, normalised and not; the learnable-temporal
class with T = 3; and the full prepare_data of a three-level pyramid (5 x 7, 3 x 4, 2 x 2; C = 16) whose three frames have a
rectangular padding, holes, and nothing valid at all.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else None
SIZES = ((5, 7), (3, 4), (2, 2))


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a placeholder class (enough for `from x import Y`)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference():
    src = os.path.join(REFERENCE, "src")
    for name, path in (("refsrc", src), ("refsrc.models", os.path.join(src, "models")), ("refsrc.util", os.path.join(src, "util"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    for name in ("pycocotools", "pycocotools.mask", "visdom", "refsrc.util.mask_ops", "refsrc.models.ops", "refsrc.models.ops.modules"):
        sys.modules.setdefault(name, _Anything(name))
    try:
        import torchvision.ops.boxes  # noqa: F401
    except ImportError:
        for name in ("torchvision", "torchvision.ops", "torchvision.ops.misc", "torchvision.ops.boxes"):
            sys.modules[name] = _Anything(name)
        sys.modules["torchvision"].__version__ = "0.0"
    encoding = importlib.import_module("refsrc.models.position_encoding")
    transformer = importlib.import_module("refsrc.models.deformable_transformer")
    assert encoding.__file__ == os.path.join(src, "models", "position_encoding.py")
    assert transformer.__file__ == os.path.join(src, "models", "deformable_transformer.py")
    return encoding, transformer


def masks_of(g, frames, h, w, kinds):
    """bool [frames, h, w]: per frame a rectangular padding ("rect"), that plus random holes ("holes") or all True ("full")."""
    mask = torch.zeros(frames, h, w, dtype=torch.bool)
    for n, kind in enumerate(kinds):
        if kind == "full":
            mask[n] = True
            continue
        mask[n, h - max(1, h // 3):, :] = True
        mask[n, :, w - max(1, w // 4):] = True
        if kind == "holes":
            mask[n] |= torch.rand(h, w, generator=g) < 0.3
    return mask


def nested(encoding, mask, channels=1):
    return sys.modules["refsrc.util.misc"].NestedTensor(torch.zeros(mask.shape[0], channels, *mask.shape[1:]), mask)


def sine_case(encoding):
    g = torch.Generator().manual_seed(1801)
    mask = masks_of(g, 2, 5, 7, ("rect", "holes"))
    d = {"mask": mask.numpy(), "num_pos_feats": np.array(8)}
    with torch.no_grad():
        d["pos_plain"] = encoding.PositionEmbeddingSine(8)(nested(encoding, mask)).numpy()
        d["pos_normalized"] = encoding.PositionEmbeddingSine(8, normalize=True)(nested(encoding, mask)).numpy()
        d["pos_scaled"] = encoding.PositionEmbeddingSine(8, temperature=20, normalize=True, scale=3.0)(nested(encoding, mask)).numpy()
    return d


def temporal_case(encoding):
    g = torch.Generator().manual_seed(1802)
    mask = masks_of(g, 3, 5, 7, ("rect", "holes", "holes"))
    module = encoding.PositionEmbeddingSineWithLearnableTemporal(16, num_frames=3, normalize=True)
    with torch.no_grad():
        module.temporal_embed.copy_(torch.randn(3, 16, generator=g))
        pos = module(nested(encoding, mask))
    assert list(module.state_dict()) == ["temporal_embed"]
    return {"mask": mask.numpy(), "temporal_embed": module.temporal_embed.detach().numpy(), "pos": pos.numpy(),
            "hidden_dim": np.array(16)}


def prepare_case(encoding, transformer):
    g = torch.Generator().manual_seed(1803)
    module = encoding.PositionEmbeddingSineWithLearnableTemporal(16, num_frames=3, normalize=True)
    top = types.SimpleNamespace(level_embed=torch.randn(3, 16, generator=g))
    top.get_valid_ratio = types.MethodType(transformer.DeformableTransformer.get_valid_ratio, top)
    masks = [masks_of(g, 3, h, w, ("rect", "holes", "full")) for h, w in SIZES]
    # whole numbers: they only travel, and compress
    srcs = [torch.arange(3 * 16 * h * w, dtype=torch.float32).reshape(3, 16, h, w) + 1000 * l for l, (h, w) in enumerate(SIZES)]
    with torch.no_grad():
        module.temporal_embed.copy_(torch.randn(3, 16, generator=g))
        pos = [module(nested(encoding, m)).to(torch.float32) for m in masks]
        out = transformer.DeformableTransformer.prepare_data(top, srcs, masks, pos)
    names = ("src_flatten", "mask_flatten", "lvl_pos_embed_flatten", "spatial_shapes", "level_start_index", "valid_ratios")
    d = {name: t.numpy() for name, t in zip(names, out)}
    d.update({"temporal_embed": module.temporal_embed.detach().numpy(), "level_embed": top.level_embed.numpy()})
    for l, (m, p) in enumerate(zip(masks, pos)):
        d["mask_%d" % l], d["pos_%d" % l] = m.numpy(), p.numpy()
    return d


def main():
    if REFERENCE is None:
        raise SystemExit(__doc__)
    encoding, transformer = import_reference()
    cases = {"posembed_sine": sine_case(encoding), "posembed_temporal": temporal_case(encoding),
             "posembed_prepare": prepare_case(encoding, transformer)}
    for name, d in sorted(cases.items()):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 32 << 10, (name, os.path.getsize(path))
        print("wrote %s (%d bytes)" % (name, os.path.getsize(path)))


if __name__ == "__main__":
    main()
