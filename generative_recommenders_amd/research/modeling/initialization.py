"""Parameter initialisers of the research path (research/modeling/initialization.py): ``truncated_normal`` -- a normal draw
kept inside mean +- 2 std -- and the Xavier-uniform / zero-bias initialiser of the MLPs."""

import torch


def truncated_normal(x: torch.Tensor, mean: float, std: float) -> torch.Tensor:
    """Fills ``x`` in place: per element four standard-normal candidates, the first one inside (-2, 2) wins (the first
    candidate when none is: probability 4e-6, clamped here so that the bound holds without exception), then ``* std + mean``."""
    with torch.no_grad():
        candidates = torch.empty(tuple(x.shape) + (4,), dtype=x.dtype, device=x.device).normal_()
        inside = (candidates > -2) & (candidates < 2)
        first = inside.to(torch.uint8).argmax(dim=-1, keepdim=True)
        x.copy_(candidates.gather(-1, first).squeeze(-1).clamp_(-2, 2))
        x.mul_(std).add_(mean)
    return x


def init_mlp_xavier_weights_zero_bias(m: torch.nn.Module) -> None:
    if isinstance(m, torch.nn.Linear):
        torch.nn.init.xavier_uniform_(m.weight)
        if getattr(m, "bias", None) is not None:
            m.bias.data.zero_()
