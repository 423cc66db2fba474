"""Records tests/golden/layerglue_*.npz from the REFERENCE's own DeformableTransformerEncoderLayer and
DeformableTransformerDecoderLayer (src/models/deformable_transformer.py), in float64 on the CPU and in eval mode:
d_model = 32, d_ffn = 64, n_points = None, so the layers build no deformable attention; the attention attribute (``self_attn`` of
the encoder layer, ``cross_attn`` of the decoder layer) is set to a stub that returns a recorded tensor.  The decoder layer's
``nn.MultiheadAttention`` (8 heads) is torch's own and runs.  Tensors only; each file under 32 KiB.

    python tests/golden/make_golden_layerglue.py /path/to/reference

The reference module is imported as make_golden_posembed.py imports it -- a package whose __init__ is skipped, with stand-ins
for what the imports pull in and never call here.

Cases: ``src`` [2, 7, 32] through the encoder layer, ``tgt`` [1, 6, 32] through the decoder layer.  Inputs, the stub's output
and the parameters hold values that are exact in float16, and are stored in float16; the outputs and the gradients -- of the
input, of the stub's output (the stub hands out a leaf) and of every parameter, for the recorded ``grad_out`` -- are the float64
results stored in float32 (a rounding of 2^-24, far below every tolerance they are compared at; float64 would not fit the size
limit).  The position tensors only reach the stub and have no gradient.  The parameter gradients have files of their
own: ``layerglue_encoder_grads``, and for the decoder layer ``layerglue_decoder_grads_attention`` (``self_attn.*``) and
``layerglue_decoder_grads_ffn`` (the rest).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else None
D_MODEL, D_FFN, HEADS = 32, 64, 8


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
    for name in ("pycocotools", "pycocotools.mask", "visdom", "refsrc.util.mask_ops", "refsrc.util.misc", "refsrc.models.ops",
                 "refsrc.models.ops.modules"):
        sys.modules.setdefault(name, _Anything(name))
    transformer = importlib.import_module("refsrc.models.deformable_transformer")
    assert transformer.__file__ == os.path.join(src, "models", "deformable_transformer.py")
    return transformer


def exact16(*shape, generator):
    """float64 values that float16 holds exactly."""
    return torch.randn(*shape, generator=generator).to(torch.float16).double()


def fill(layer, generator):
    """Parameters exact in float16; the norms away from (1, 0) so that weight and bias matter."""
    with torch.no_grad():
        for name, p in layer.named_parameters():
            scale = 0.25 if p.dim() > 1 or "proj" in name or "linear" in name else 1.0
            offset = 1.0 if name.startswith("norm") and name.endswith("weight") else 0.0
            p.copy_((exact16(*p.shape, generator=generator) * scale + offset).to(torch.float16).double())


def record(layer, inputs, attention, out, grad_out):
    """The tensors of one case; gradients of inputs[0], the stub's output and every parameter."""
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(out, [inputs[0][1], attention] + list(params.values()), grad_out)
    half = lambda t: t.detach().to(torch.float16).numpy()      # noqa: E731
    single = lambda t: t.detach().to(torch.float32).numpy()    # noqa: E731
    for t in [v for _, v in inputs] + [attention] + list(params.values()):
        assert torch.equal(t.detach().to(torch.float16).double(), t.detach()), "not exact in float16"
    d = {name: half(t) for name, t in inputs}
    d.update({"attention": half(attention), "grad_out": half(grad_out), "out": single(out)})
    d.update({"state." + name: half(t) for name, t in layer.state_dict().items()})
    d["grad." + inputs[0][0]], d["grad.attention"] = single(grads[0]), single(grads[1])
    param_grads = {"grad." + name: single(g) for name, g in zip(params, grads[2:])}
    return d, param_grads


def encoder_case(transformer):
    g = torch.Generator().manual_seed(1901)
    layer = transformer.DeformableTransformerEncoderLayer(d_model=D_MODEL, d_ffn=D_FFN, n_heads=HEADS, n_points=None).double().eval()
    fill(layer, g)
    src, pos = exact16(2, 7, D_MODEL, generator=g).requires_grad_(True), exact16(2, 7, D_MODEL, generator=g)
    attention = exact16(2, 7, D_MODEL, generator=g).requires_grad_(True)
    layer.self_attn = lambda *args, **kwargs: (attention, None)
    out = layer(src, pos, None, None, None)
    d, param_grads = record(layer, [("src", src), ("pos", pos)], attention, out, exact16(2, 7, D_MODEL, generator=g))
    return {"layerglue_encoder": d, "layerglue_encoder_grads": param_grads}


def decoder_case(transformer):
    g = torch.Generator().manual_seed(1902)
    layer = transformer.DeformableTransformerDecoderLayer(d_model=D_MODEL, d_ffn=D_FFN, n_heads=HEADS, n_points=None).double().eval()
    fill(layer, g)
    tgt, query_pos = exact16(1, 6, D_MODEL, generator=g).requires_grad_(True), exact16(1, 6, D_MODEL, generator=g)
    attention = exact16(1, 6, D_MODEL, generator=g).requires_grad_(True)
    layer.cross_attn = lambda *args, **kwargs: (attention, None)
    out = layer(tgt, query_pos, None, None, None, None)
    d, param_grads = record(layer, [("tgt", tgt), ("query_pos", query_pos)], attention, out, exact16(1, 6, D_MODEL, generator=g))
    return {"layerglue_decoder": d,
            "layerglue_decoder_grads_attention": {k: v for k, v in param_grads.items() if k.startswith("grad.self_attn.")},
            "layerglue_decoder_grads_ffn": {k: v for k, v in param_grads.items() if not k.startswith("grad.self_attn.")}}


def main():
    if REFERENCE is None:
        raise SystemExit(__doc__)
    transformer = import_reference()
    cases = dict(encoder_case(transformer))
    cases.update(decoder_case(transformer))
    for name, d in sorted(cases.items()):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 32 << 10, (name, os.path.getsize(path))
        print("wrote %s (%d bytes)" % (name, os.path.getsize(path)))


if __name__ == "__main__":
    main()
