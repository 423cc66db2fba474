"""What the CPU and GPU tests of the transformer layers' glue share (tests/ only): stand-ins for the reference's layer classes
-- its attribute names, its chain restated in torch -- and the layerglue_* fixtures recorded from the reference's own classes
(tests/golden/make_golden_layerglue.py)."""
import types

import torch
import torch.nn.functional as F
from torch import nn

from conftest import golden

D_MODEL, D_FFN, HEADS = 32, 64, 8
GRAD_FILES = {"encoder": ("layerglue_encoder_grads",),
              "decoder": ("layerglue_decoder_grads_attention", "layerglue_decoder_grads_ffn")}


class StockEncoderLayer(nn.Module):
    """The attributes of DeformableTransformerEncoderLayer (n_points=None: no attention module is built) and what its two
    methods compute."""

    def __init__(self, d_model=D_MODEL, d_ffn=D_FFN, dropout=0.1, n_heads=HEADS):
        super().__init__()
        self.self_attn = None
        self.dropout1, self.norm1 = nn.Dropout(dropout), nn.LayerNorm(d_model)
        self.linear1, self.activation, self.dropout2 = nn.Linear(d_model, d_ffn), F.relu, nn.Dropout(dropout)
        self.linear2, self.dropout3, self.norm2 = nn.Linear(d_ffn, d_model), nn.Dropout(dropout), nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, src):
        hidden = self.dropout2(self.activation(self.linear1(src)))
        return self.norm2(src + self.dropout3(self.linear2(hidden)))

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, **kwargs):
        attended = self.self_attn(self.with_pos_embed(src, pos), reference_points, src, spatial_shapes, level_start_index, **kwargs)[0]
        return self.forward_ffn(self.norm1(src + self.dropout1(attended)))


class StockDecoderLayer(nn.Module):
    """The attributes of DeformableTransformerDecoderLayer and what its two methods compute."""

    def __init__(self, d_model=D_MODEL, d_ffn=D_FFN, dropout=0.1, n_heads=HEADS):
        super().__init__()
        self.cross_attn = None
        self.dropout1, self.norm1 = nn.Dropout(dropout), nn.LayerNorm(d_model)
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.dropout2, self.norm2 = nn.Dropout(dropout), nn.LayerNorm(d_model)
        self.linear1, self.activation, self.dropout3 = nn.Linear(d_model, d_ffn), F.relu, nn.Dropout(dropout)
        self.linear2, self.dropout4, self.norm3 = nn.Linear(d_ffn, d_model), nn.Dropout(dropout), nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, tgt):
        hidden = self.dropout3(self.activation(self.linear1(tgt)))
        return self.norm3(tgt + self.dropout4(self.linear2(hidden)))

    def forward(self, tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index, **kwargs):
        q = self.with_pos_embed(tgt, query_pos).transpose(0, 1)
        tgt = self.norm2(tgt + self.dropout2(self.self_attn(q, q, tgt.transpose(0, 1))[0].transpose(0, 1)))
        attended = self.cross_attn(self.with_pos_embed(tgt, query_pos), reference_points, src, src_spatial_shapes,
                                   level_start_index, **kwargs)[0]
        return self.forward_ffn(self.norm1(tgt + self.dropout1(attended)))


def reference_module():
    """A ``deformable_transformer`` namespace with fresh stand-in classes, as the patches take it."""
    encoder_layer = type("DeformableTransformerEncoderLayer", (StockEncoderLayer,), {
        "forward": StockEncoderLayer.forward, "forward_ffn": StockEncoderLayer.forward_ffn})
    decoder_layer = type("DeformableTransformerDecoderLayer", (StockDecoderLayer,), {
        "forward": StockDecoderLayer.forward, "forward_ffn": StockDecoderLayer.forward_ffn})
    encoder = type("DeformableTransformerEncoder", (), {"get_reference_points": staticmethod(lambda *a: "theirs")})
    top = type("DeformableTransformer", (), {"prepare_data": lambda self, *a: "theirs"})
    return types.SimpleNamespace(DeformableTransformerEncoderLayer=encoder_layer, DeformableTransformerDecoderLayer=decoder_layer,
                                 DeformableTransformerEncoder=encoder, DeformableTransformer=top)


def load_case(kind):
    """The fixture of ``kind`` ("encoder" / "decoder") with its parameter gradients merged in, as float64 CPU tensors."""
    d = dict(golden("layerglue_" + kind))
    for name in GRAD_FILES[kind]:
        d.update(golden(name))
    return {k: torch.from_numpy(v).double() for k, v in d.items()}


def build_layer(module, kind, case, device="cpu", dtype=torch.float64, dropout=0.1):
    """(layer in eval mode holding the fixture's parameters, its inputs, the leaf its attention stub returns)."""
    cls = module.DeformableTransformerEncoderLayer if kind == "encoder" else module.DeformableTransformerDecoderLayer
    layer = cls(D_MODEL, D_FFN, dropout, n_heads=HEADS)
    layer.load_state_dict({k[len("state."):]: v for k, v in case.items() if k.startswith("state.")})
    layer = layer.to(device=device, dtype=dtype).eval()
    to = lambda t: t.to(device=device, dtype=dtype)      # noqa: E731
    attention = to(case["attention"]).requires_grad_(True)
    stub = lambda *args, **kwargs: (attention, None)     # noqa: E731
    if kind == "encoder":
        layer.self_attn = stub
        inputs = (to(case["src"]).requires_grad_(True), to(case["pos"]), None, None, None)
    else:
        layer.cross_attn = stub
        inputs = (to(case["tgt"]).requires_grad_(True), to(case["query_pos"]), None, None, None, None)
    return layer, inputs, attention


def run_case(module, kind, case, device="cpu", dtype=torch.float64):
    """{"out", "grad.<input>", "grad.attention", "grad.<parameter>"} of the layer of ``module`` on the fixture."""
    layer, inputs, attention = build_layer(module, kind, case, device, dtype)
    out = layer(*inputs)
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(out, [inputs[0], attention] + list(params.values()), case["grad_out"].to(device=device, dtype=dtype))
    got = {"out": out.detach(), "grad." + ("src" if kind == "encoder" else "tgt"): grads[0], "grad.attention": grads[1]}
    got.update({"grad." + name: g for name, g in zip(params, grads[2:])})
    return got
