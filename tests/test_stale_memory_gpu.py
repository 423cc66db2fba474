"""GPU: the operators that allocate every output and workspace with ``torch.empty`` -- deformable convolution, mask-head
stage, mask loss, box matching, assignment, label loss, position embedding -- on stale memory.  In a test process a fresh
allocation is often zero; in training the caching allocator hands back what the last tensor left.  Each case runs forward and
backward once plainly and once with tests/stale_memory.py in the place of ``torch`` in the operator's host code, on the same
inputs: every buffer is then prefilled with NaNs (0x7f bytes for the integer kinds) between two guard zones.

All of these operators document bitwise reproducibility, so every returned tensor and gradient must have the bits of the
plain run and no NaN -- an element the kernels skip, or a workspace record read before it is written, breaks that -- and
every guard byte must be intact.  The one exception is the deformable convolution's default ``grad_input``, a sum of float
atomics: it is held to test_dcn_gpu's tolerance against that file's oracle, as test_dcn_gpu holds it.  Each case also
asserts that the shim handed out at least the buffers the host code shows for the call: a test that patches nothing fails.

The custom ops' fake implementations in devis_amd/ops.py allocate too, but no eager call reaches them."""
import numpy as np
import pytest
import torch

import stale_memory

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def assert_same_bits(plain, stale, what, skip=()):
    assert len(plain) == len(stale), what
    for k, (a, b) in enumerate(zip(plain, stale)):
        assert (a is None) == (b is None), (what, k)
        if a is None or k in skip:
            continue
        assert a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride(), (what, k)
        if b.is_floating_point():
            assert not bool(torch.isnan(b).any()), (what, k, "NaN: stale memory came through")
        assert torch.equal(_bits(a), _bits(b)), (what, k, "differs from the run on fresh memory")


def on_stale_memory(monkeypatch, modules, call, at_least, what, skip=()):
    """``call()`` -> a sequence of tensors (or None), plainly and under the shim; returns (plain, stale)."""
    plain = call()
    with monkeypatch.context() as patch:
        shim = stale_memory.install(patch, modules)
        stale = call()
        torch.cuda.synchronize()
    assert len(shim.buffers) >= at_least, (what, "the shim handed out %d buffers, the host code shows %d" % (len(shim.buffers), at_least))
    assert_same_bits(plain, stale, what, skip)
    assert shim.guards_intact(), (what, "a guard zone was written")
    return plain, stale


# ---- label loss ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_label_loss_with_two_tiles(dtype, monkeypatch):
    from devis_amd import _labelloss, _native
    from devis_amd.functions import label_loss
    from test_labelloss_gpu import case, run_op, shape_of
    ops, _ = case("tile+row", dtype)
    B, N, C, M = shape_of("tile+row")
    assert _labelloss.workspace_bytes(_native.dtype_code(dtype), _labelloss.Shape(B * N, C, M)) > 0        # the tile records
    # focal_sum, counts, target_classes, the workspace; grad_logits
    on_stale_memory(monkeypatch, [label_loss], lambda: run_op(*ops), 5, "label loss %s" % dtype)


# ---- mask loss -------------------------------------------------------------------------------------------------------------

def test_mask_loss_with_two_tiles_each_way_and_with_column_chunks(monkeypatch):
    from devis_amd import _maskloss, _native
    from devis_amd.functions import mask_losses
    from test_maskloss_gpu import _tiles, grads_for, make_case, run_op
    chunk = _tiles()[4]
    for N, hw, HW, seed in ((4, (12, 20), (45, 96), 0), (2, (2, 1), (2, chunk + 905), 3)):
        src, target = make_case(N, hw, HW, seed=seed)
        grads = grads_for(N)
        partials = _maskloss.workspace_bytes(_native.dtype_code(src.dtype), _maskloss.Shape(N, *hw, *HW)) > 0
        assert partials or N == 2
        # focal, dice, sums, the partials beyond one tile; grad_src
        on_stale_memory(monkeypatch, [mask_losses], lambda: run_op(src, target, grads=grads), 5 if partials else 4,  # noqa: B023
                        "mask loss %s -> %s" % (hw, HW))


# ---- position embedding ----------------------------------------------------------------------------------------------------

def test_position_embedding_forward_backward_and_one_level(monkeypatch):
    import devis_amd
    from devis_amd.functions import position_embedding
    from test_posembed_gpu import backward_case, gradients, on_device, reference, run
    r = reference("pyramid")
    # the counts workspace, mask_flatten, valid_ratios, pos
    plain, _ = on_stale_memory(monkeypatch, [position_embedding], lambda: run(r), 4, "pyramid float32")
    assert plain[1].dtype == torch.bool and plain[0].dtype == torch.float32
    low = dict(round_dtype=torch.bfloat16, out_dtype=torch.bfloat16)
    plain, _ = on_stale_memory(monkeypatch, [position_embedding], lambda: run(r, **low), 4, "pyramid bfloat16")
    assert plain[0].dtype == torch.bfloat16
    # ... and grad_level_embed, grad_temporal_embed, the partial sums: two channel blocks
    case = backward_case("c72", exact=False)
    on_stale_memory(monkeypatch, [position_embedding], lambda: gradients(*case), 7, "backward c72")
    # [N, C, H, W] of one level: pos, the counts workspace
    mask = on_device(r)[0][0]
    sine = lambda: (devis_amd.sine_position_embedding(mask, num_pos_feats=8, normalize=True),)      # noqa: E731
    on_stale_memory(monkeypatch, [position_embedding], sine, 2, "one level")


# ---- box matching ----------------------------------------------------------------------------------------------------------

def test_match_cost_and_box_loss_terms(monkeypatch):
    import devis_amd
    from devis_amd.functions import box_matching
    from test_boxmatch_gpu import WEIGHTS, boxes_of, cost_case, on_gpu
    ops = on_gpu(cost_case((3, 6, 50, 9, 40), torch.float32)[0])
    # cost, status
    plain, _ = on_stale_memory(monkeypatch, [box_matching], lambda: devis_amd.match_cost(*ops, **WEIGHTS), 2, "match_cost")
    assert plain[1].tolist() == [0, 0, 0]
    g = torch.Generator().manual_seed(300)
    src, target = boxes_of(g, 300).float().to(DEV), boxes_of(g, 300).float().to(DEV)
    grads = [torch.randn(300, generator=g).to(DEV), torch.randn(300, generator=g).to(DEV)]

    def terms():
        s = src.clone().requires_grad_(True)
        l1, giou = devis_amd.box_loss_terms(s, target)
        return l1.detach(), giou.detach(), torch.autograd.grad([l1, giou], s, grads)[0]

    # l1, giou; grad_src
    on_stale_memory(monkeypatch, [box_matching], terms, 3, "box_loss_terms")


# ---- assignment ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(150, 150), (130, 90)], ids=lambda s: "x".join(map(str, s)))
def test_assignment_of_three_problems_one_of_them_invalid(shape, monkeypatch):
    import devis_amd
    from devis_amd.functions import assignment
    from test_assign_cpu import generic_case
    batch = np.stack([generic_case(shape, k)[0] for k in range(3)])
    batch[1, 3, 5] = np.nan                 # the identity pairs of an invalid problem are written too
    cost = torch.from_numpy(batch).to(DEV)
    # rows, cols, status
    plain, _ = on_stale_memory(monkeypatch, [assignment], lambda: devis_amd.linear_assignment(cost), 3, shape)
    rows, cols, status = plain
    assert status.tolist() == [1, 0] and rows[1].tolist() == cols[1].tolist() == list(range(min(shape)))
    for k in (0, 2):
        want = generic_case(shape, k)[1]
        assert rows[k].tolist() == want[0].tolist() and cols[k].tolist() == want[1].tolist()


# ---- mask-head stage -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage", [(6, 3, 128, 8, 8, (5, 7), (9, 14)), (4, 2, 32, 8, 0, (7, 5), (14, 10))], ids=["c128+extra", "c32"])
def test_mask_head_stage_with_full_backward(stage, monkeypatch):
    from devis_amd.functions import _common, mask_head_stage
    from test_mhstage_gpu import NAMES, STAGES, grad_out_for, make_case, run_op
    assert stage in STAGES
    d = make_case(*stage, torch.float32)
    go = grad_out_for(d, torch.float32).to(DEV)

    def call():
        out, grads = run_op(d, go)
        assert sorted(grads) == sorted(k for k in NAMES if d[k] is not None)
        return [out] + [grads.get(k) for k in NAMES]

    # out, mean, rstd, the forward's workspace; grad_weight, grad_bias, grad_skip, dy (grad_x in float32), the backward's
    plain, stale = on_stale_memory(monkeypatch, [mask_head_stage, _common], call, 9, stage)
    assert stale[0].is_contiguous(memory_format=torch.channels_last)


# ---- deformable convolution ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reproducible", [False, True], ids=["float atomics", "reproducible_grad_input"])
def test_deformable_convolution_forward_and_backward(reproducible, monkeypatch):
    import devis_amd
    from devis_amd import ops
    from devis_amd.functions import deform_conv
    from test_dcn_gpu import TOL, assert_close, hip, make_inputs, oracle
    tensors, geometry = make_inputs(N=4, C=72, Co=32, H=23, W=40)
    # out, the columns; grad_offset, grad_mask, grad_columns, the columns, grad_input, grad_weight; with the fixed-point sum its
    # accumulator and its workspace as well
    if reproducible:
        with devis_amd.reproducible_grad_input():
            on_stale_memory(monkeypatch, [deform_conv, ops], lambda: hip(tensors, geometry), 10, "reproducible")
    else:
        plain, stale = on_stale_memory(monkeypatch, [deform_conv, ops], lambda: hip(tensors, geometry), 8, "default", skip=(1,))
        assert not bool(torch.isnan(stale[1]).any())
        want = oracle(tensors, geometry)
        assert_close(stale, want, TOL[torch.float32], "stale memory")
        assert_close(plain, want, TOL[torch.float32], "fresh memory")
