"""CPU restatement of the symmetry augmentation in torch's own ops (the definition, not the index formulas)."""
import torch


def augment_one(x: torch.Tensor, g: int, dy: int, dx: int) -> torch.Tensor:
    """One [H, H] map under the op (g, dy, dx): flip, quarter turns, roll."""
    f, r = g >> 2, g & 3
    x = x.flip(-1) if f else x
    x = torch.rot90(x, r, (-2, -1))
    x = torch.roll(x, (dy, dx), (-2, -1))
    return x


def augment_ref(x: torch.Tensor, ops) -> torch.Tensor:
    """x [B, H, H] or [B, 1, H, H] (any device) and ops [B, 3]: the augmented batch on the CPU, in x's shape."""
    xc = x.detach().cpu()
    maps = xc.reshape(xc.shape[0], xc.shape[-2], xc.shape[-1])
    o = torch.as_tensor(ops).cpu().tolist()
    out = torch.stack([augment_one(m, *op) for m, op in zip(maps, o)])
    return out.reshape(xc.shape).contiguous()
