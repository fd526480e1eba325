"""The plane-buffer rule of the mask-family losses (loss._planes_base), which needs no GPU: the network's own (..., S) buffer when
the masks are exactly its planes, a fresh ``torch.stack`` otherwise."""
import pytest
import torch

SHAPE = (2, 3, 5)


def _buffer(S, dtype=torch.float32, planes=None):
    g = torch.Generator().manual_seed(11 * S)
    return torch.rand(*SHAPE, planes or S, generator=g).to(dtype)


def _is_fresh_stack(got, masks, *buffers):
    S = len(masks)
    assert got.shape == (*SHAPE, S) and got.dtype == torch.float32 and got.is_contiguous()
    assert all(got.data_ptr() != b.data_ptr() for b in buffers)
    assert got._base is None
    for k, m in enumerate(masks):
        assert torch.equal(got[..., k], m.float())


@pytest.mark.parametrize("S", [2, 3, 4])
def test_planes_of_the_network_buffer_are_taken_as_they_lie(S):
    from onssen_amd.loss import _planes_base
    buf = _buffer(S)
    got = _planes_base([buf[..., k] for k in range(S)])
    assert got.data_ptr() == buf.data_ptr() and got.shape == (*SHAPE, S)
    assert torch.equal(got, buf)
    # the head's flat (B, T, F S) output, viewed and sliced as the networks do
    flat = _buffer(S).view(SHAPE[0], SHAPE[1], SHAPE[2] * S).clone()          # a root tensor of its own, as the head's output is
    got = _planes_base([flat.view(*SHAPE, S)[..., k] for k in range(S)])
    assert got.data_ptr() == flat.data_ptr() and got.shape == (*SHAPE, S)
    assert torch.equal(got, flat.view(*SHAPE, S))


@pytest.mark.parametrize("S", [2, 3, 4])
def test_anything_else_is_stacked(S):
    from onssen_amd.loss import _planes_base
    buf, other = _buffer(S), _buffer(S) + 1
    swapped = [buf[..., k] for k in range(S)]
    swapped[0], swapped[1] = swapped[1], swapped[0]
    _is_fresh_stack(_planes_base(swapped), swapped, buf)
    mixed = [buf[..., 0]] + [other[..., k] for k in range(1, S)]
    _is_fresh_stack(_planes_base(mixed), mixed, buf, other)
    half = _buffer(S, torch.float16)
    masks = [half[..., k] for k in range(S)]
    _is_fresh_stack(_planes_base(masks), masks, half)
    wide = _buffer(S, planes=S + 1)
    masks = [wide[..., k] for k in range(S)]
    _is_fresh_stack(_planes_base(masks), masks, wide)
    # a contiguous slice at a non-zero offset of a larger tensor: its planes are consistent among themselves, but a view's _base
    # is the root tensor, which has more than S * numel elements -- stacked, as loss._upit_masks_base decided before this helper
    big = torch.stack([_buffer(S), _buffer(S) + 2])
    part = big[1]
    assert part.storage_offset() > 0 and part.is_contiguous()
    masks = [part[..., k] for k in range(S)]
    _is_fresh_stack(_planes_base(masks), masks, big, part)
    masks = [_buffer(S)[..., k].contiguous() for k in range(S)]
    _is_fresh_stack(_planes_base(masks), masks, *masks)


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("flat", [False, True])
def test_gradient_reaches_the_leaf_buffer_in_its_own_shape(S, flat):
    from onssen_amd.loss import _planes_base
    leaf = _buffer(S)
    if flat:
        leaf = leaf.view(SHAPE[0], SHAPE[1], SHAPE[2] * S).clone()
    leaf.requires_grad_(True)
    planes = leaf.view(*SHAPE, S)
    got = _planes_base([planes[..., k] for k in range(S)])
    assert got.data_ptr() == leaf.data_ptr()
    got.sum().backward()
    assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, torch.ones_like(leaf))
