"""RoPE2dV2: mirror of the reference's src/blocks/rotary_embedding_2d_v2.py (positional_encoding="RoPE2dV2", Attention.py:105-107,
220-239).  Channel triples (3j, 3j+1, 3j+2) of a head vector are rotated by two angles -- theta_j from the token's row on the patch grid,
alpha_j from its column -- and the three rotated components are written as three concatenated groups [0, T), [T, 2T), [2T, 3T) with
T = dim // 3; channels from 3T on pass through.  On the HIP path the rotation runs inside mmdit_qk_norm_rope3_fwd / _bwd
(csrc/rowops_rope3.hip); this module owns the `inv_freq` buffer (it is part of the reference's state_dict) and builds the cos / sin tables.
forward() is a host-side utility with the reference's semantics."""
import torch
from torch import nn


class RoPE2D(nn.Module):
    def __init__(self, dim, interpolate_factor=1):
        super().__init__()
        self.triples = dim // 3
        self.dim = 3 * self.triples
        # 10000^(-j / T) as the reference rounds it: the exponent is (3j) / (3T) in fp32
        self.register_buffer("inv_freq", 1.0 / (10000 ** (torch.arange(0, self.dim, 3).float() / self.dim)))
        self.interpolate_factor = interpolate_factor
        self._tables = {}

    def _angles(self, height, width):
        """theta (height, T) and alpha (width, T) in fp32, in the reference's order of operations: (index / factor) * inv_freq."""
        fr = self.inv_freq.detach().float().cpu()
        rows = torch.arange(height).float()[:, None] / self.interpolate_factor
        cols = torch.arange(width).float()[:, None] / self.interpolate_factor
        return rows * fr, cols * fr

    def tables(self, height, width, device):
        """(cos, sin), each (height*width, 2T) fp32 on `device`: [theta part | alpha part] of token n = row * width + column.  Cached per
        shape and buffer version."""
        key = (height, width, str(device), self.inv_freq._version, self.inv_freq.data_ptr(), self.interpolate_factor)
        tb = self._tables.get(key)
        if tb is None:
            th, al = self._angles(height, width)
            T = th.shape[-1]
            ang = torch.cat([th[:, None, :].expand(height, width, T), al[None, :, :].expand(height, width, T)], dim=-1).reshape(height * width, 2 * T)
            tb = (ang.cos().contiguous().to(device), ang.sin().contiguous().to(device))
            self._tables = {key: tb}
        return tb

    def forward(self, x):
        """x (batch, heads, height, width, head_dim): rotates the first 3T channels IN PLACE (as the reference does) and returns x."""
        n = 3 * (x.shape[-1] // 3)
        with torch.no_grad():
            fr = self.inv_freq.to(x.device)
            th = (torch.arange(x.shape[2], device=x.device).float()[:, None] / self.interpolate_factor * fr)[None, None, :, None, :]
            al = (torch.arange(x.shape[3], device=x.device).float()[:, None] / self.interpolate_factor * fr)[None, None, None, :, :]
            ct, st, ca, sa = th.cos(), th.sin(), al.cos(), al.sin()
        a, b, d = x[..., 0:n:3], x[..., 1:n:3], x[..., 2:n:3]
        rot = torch.cat([a * ct + b * -st * ca + d * st * sa,
                         a * st + b * ct * ca + d * -ct * sa,
                         b * sa + d * ca], dim=-1)
        x[..., :n] = rot
        return x

    def __deepcopy__(self, memo):
        import copy
        new = RoPE2D.__new__(RoPE2D)
        nn.Module.__init__(new)
        new.triples, new.dim, new.interpolate_factor = self.triples, self.dim, self.interpolate_factor
        new.register_buffer("inv_freq", copy.deepcopy(self.inv_freq, memo))
        new._tables = {}
        return new
