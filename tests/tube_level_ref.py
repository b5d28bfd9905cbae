"""Test-only float64-capable restatement of the level-conditioned tube loss: the pinball loss of
tests/tube_ref.py with one level per ROW, shape (B, 1), in place of the scalar alpha.  This is the intended semantics; the
reference's AlphaScalarTubeLoss takes alpha = data[:, -1] of shape (B,), which broadcasts against the (B, 1) residual to B x B."""
import torch


def pinball(fw, w, level):
    """fw, w (B, O); level (B, 1)."""
    assert level.dim() == 2 and level.shape == (fw.shape[0], 1)
    r = w - fw
    return torch.where(r > 0, level * r, (1 - level) * r.abs())


def loss(name, fw, w, level, delta=1.0):
    """scalar_level: Huber(delta) of every element's pinball value, mean over elements.  vector_level: the pinball values summed
    per row, then Huber, mean over rows."""
    l = pinball(fw, w, level)
    if name == "vector_level":
        l = l.sum(dim=-1)
    elif name != "scalar_level":
        raise ValueError(name)
    return torch.nn.functional.huber_loss(l, torch.zeros_like(l), delta=delta)
