"""What the window-attention tests share (tests/ only): the shape cases, rounded inputs, and a reference-shaped Swin stage --
``Mlp``, ``WindowAttention``, ``SwinTransformerBlock`` and ``BasicLayer`` with the attribute names, parameter names and call
signatures of the reference's ``src/models/swin_backbone.py`` (``timm`` is not a dependency, so the reference's classes cannot
be imported) -- written anew, with the window attention as tests/winattn_oracle.py computes it, the mask built once per stage
and handed to the blocks as ``mask_matrix``.  This module stands in for ``src.models.swin_backbone`` in
``devis_amd.patch_window_attention(winattn_cases)``.  The fixture tests/golden/winattn_*.npz was recorded from the reference's
own ``BasicLayer`` (tests/golden/make_golden_winattn.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint
from torch import nn

import winattn_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)

# (ws, shift, Hp, Wp, B, nH, D)
SHAPES = [
    (4, 0, 4, 4, 1, 1, 4),              # one window of exactly one tile
    (4, 1, 4, 4, 1, 1, 4),              # every mask region inside one window
    (5, 2, 10, 15, 2, 2, 20),           # a row tail of 9
    (7, 3, 14, 21, 2, 2, 32),           # three full tiles plus a tile of a single row; the reference's window
    (7, 3, 7, 14, 1, 3, 32),            # one window row
    (12, 6, 12, 24, 1, 1, 32),          # N = 144
    (2, 1, 4, 6, 3, 2, 64),             # small window, largest head dimension
]
UNSHIFTED = [(ws, 0) + tuple(rest) for ws, shift, *rest in SHAPES if shift and (ws, 0) + tuple(rest) not in SHAPES]
SHAPES_16 = [SHAPES[2], SHAPES[3]]      # bfloat16 and float16, with a float32 table
CHUNKED = (2, 1, 34, 38, 1, 1, 4)       # 323 windows: grad_table's first pass sums them in 162 chunks of two, the last of one
LAYER = dict(dim=16, depth=2, num_heads=2, window_size=4, mlp_ratio=2.0)        # the recorded stage
LAYER_INPUT = (2, 6, 9)                 # B, H, W: the padded map is 8 x 12


def case_id(case):
    return "ws%d-shift%d-%dx%d-B%d-H%d-D%d" % tuple(case)


def make_inputs(case, dtype=torch.float32, table_dtype=None, seed=0, gain=1.0):
    """(qkv [B, Hp, Wp, 3C], table [(2 ws - 1)^2, nH], grad_out [B, Hp, Wp, C]) on the CPU, rounded to their dtypes.  ``gain``
    scales q, so that the softmax is peaked."""
    ws, shift, Hp, Wp, B, H, D = case
    g = torch.Generator().manual_seed(1000 + seed)
    C = H * D
    qkv = torch.randn(B, Hp, Wp, 3, C, generator=g)
    qkv[:, :, :, 0] *= gain
    table = torch.randn((2 * ws - 1) ** 2, H, generator=g)
    grad_out = torch.randn(B, Hp, Wp, C, generator=g)
    return qkv.reshape(B, Hp, Wp, 3 * C).to(dtype), table.to(table_dtype or dtype), grad_out.to(dtype)


# ---- a reference-shaped stage ----------------------------------------------------------------------------------------------

class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features, drop=0.0):
        super().__init__()
        self.fc1, self.act, self.fc2, self.drop = nn.Linear(in_features, hidden_features), nn.GELU(), nn.Linear(hidden_features, in_features), nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class WindowAttention(nn.Module):
    """Attention over the tokens of windows [windows * B, N, C] with a relative-position bias and an optional additive mask."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        assert window_size[0] == window_size[1]
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        self.register_buffer("relative_position_index", O.relative_rows(window_size[0]).clone())
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.softmax = nn.Softmax(dim=-1)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def forward(self, x, mask=None):
        windows, N, C = x.shape
        H = self.num_heads
        q, k, v = self.qkv(x).reshape(windows, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
        logits = (q * self.scale) @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.reshape(-1)].reshape(N, N, H)
        logits = logits + bias.permute(2, 0, 1)[None]
        if mask is not None:
            per_map = mask.shape[0]
            logits = (logits.reshape(windows // per_map, per_map, H, N, N) + mask[None, :, None]).reshape(windows, H, N, N)
        x = (self.attn_drop(self.softmax(logits)) @ v).transpose(1, 2).reshape(windows, N, C)
        return self.proj_drop(self.proj(x))


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0):
        super().__init__()
        assert 0 <= shift_size < window_size
        self.dim, self.num_heads, self.window_size, self.shift_size, self.mlp_ratio = dim, num_heads, window_size, shift_size, mlp_ratio
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, (window_size, window_size), num_heads, qkv_bias, qk_scale, attn_drop, drop)
        self.drop_path = nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), drop)
        self.H = self.W = None

    def forward(self, x, mask_matrix):
        B, L, C = x.shape
        H, W, ws, shift = self.H, self.W, self.window_size, self.shift_size
        assert L == H * W
        shortcut = x
        x = F.pad(self.norm1(x).view(B, H, W, C), (0, 0, 0, -W % ws, 0, -H % ws))
        Hp, Wp = x.shape[1:3]
        if shift:
            x = torch.roll(x, (-shift, -shift), (1, 2))
        tokens = O.partition(x, ws).reshape(-1, ws * ws, C)
        tokens = self.attn(tokens, mask=mask_matrix if shift else None)
        x = O.reverse(tokens.reshape(B, -1, ws * ws, C), ws, Hp, Wp)
        if shift:
            x = torch.roll(x, (shift, shift), (1, 2))
        x = x[:, :H, :W].reshape(B, H * W, C)
        x = shortcut + self.drop_path(x)
        return x + self.drop_path(self.mlp(self.norm2(x)))


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4.0, use_checkpoint=False, attn_drop=0.0):
        super().__init__()
        self.window_size, self.shift_size, self.depth, self.use_checkpoint = window_size, window_size // 2, depth, use_checkpoint
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2,
                                                          mlp_ratio, attn_drop=attn_drop) for i in range(depth)])
        self.downsample = None

    def forward(self, x, H, W):
        ws = self.window_size
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        attn_mask = O.sliced_mask(Hp, Wp, ws, self.shift_size).to(device=x.device, dtype=x.dtype)
        for blk in self.blocks:
            blk.H, blk.W = H, W
            x = checkpoint.checkpoint(blk, x, attn_mask, use_reentrant=False) if self.use_checkpoint else blk(x, attn_mask)
        return x, H, W, x, H, W


# ---- the fixture -------------------------------------------------------------------------------------------------------------

def load_fixture():
    """{name: float64 tensor} of tests/golden/winattn_layer.npz and its gradient files."""
    case = {}
    for name in ("winattn_layer", "winattn_layer_out", "winattn_layer_grads_block0", "winattn_layer_grads_block1"):
        with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
            case.update({k: torch.from_numpy(f[k].astype(np.float64) if f[k].dtype.kind == "f" else f[k]) for k in f.files})
    return case


def build_layer(case, dtype=torch.float64, device="cpu", **kwargs):
    """The recorded stage with the fixture's state dict, and its input (a leaf)."""
    layer = BasicLayer(**LAYER, **kwargs).to(dtype)
    state = {k[len("state."):]: v for k, v in case.items() if k.startswith("state.")}
    assert sorted(state) == sorted(layer.state_dict())
    layer.load_state_dict(state)
    layer = layer.to(device).eval()
    x = case["x"].to(device=device, dtype=dtype).requires_grad_(True)
    return layer, x


def run_layer(layer, x, case):
    """{"out", "grad.x", "grad.<parameter>"} of one forward and backward of the recorded stage."""
    B, H, W = LAYER_INPUT
    out = layer(x, H, W)[0]
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(out, [x] + list(params.values()), case["grad_out"].to(device=out.device, dtype=out.dtype))
    got = {"out": out.detach(), "grad.x": grads[0]}
    got.update({"grad." + name: g for name, g in zip(params, grads[1:])})
    return got
