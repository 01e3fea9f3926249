"""Derivative fields of a decoded signal: the Jacobian of the field w.r.t. the query coordinates from the native call
(EquivariantCrossAttentionNeF.jacobian, include/enf_hip.h: enf_field_grad) and the first-order operators built on it.

  decode_jacobian(...)   the counterpart of inner_loop.decode: (out, jac) on the full grid, chunking optional
  divergence / curl_2d / gradient_norm   operators on a Jacobian whose components are CARTESIAN

The Jacobian is w.r.t. the coordinates as the model takes them.  For the planar invariants these are Cartesian and the operators
below are the usual ones; for the spherical and ball invariants they are angles (and a radius), and a divergence or curl needs
the metric factors, which are not applied here.
"""
import torch

__all__ = ["decode_jacobian", "divergence", "curl_2d", "gradient_norm"]


def decode_jacobian(nef, nef_params, coords, p, a, window, chunk=None):
    """(out (B, N, O), jac (B, N, O, dx)) on the full grid: jac[b, n, o, i] = d out[b, n, o] / d coords[n, i], per signal.
    ``coords`` (N, dx) is one grid shared by the batch, or (B, N, dx).  ``chunk``: decode that many points at a time (slices of the
    grid; the per-chunk results are concatenated along N) -- the native call tiles over queries itself, so this only bounds the
    workspace."""
    B = p.shape[0]
    x = coords[None].expand(B, -1, -1) if coords.dim() == 2 else coords
    if chunk is None:
        return nef.jacobian(nef_params, x, p, a, window)
    parts = [nef.jacobian(nef_params, x[:, i:i + chunk], p, a, window) for i in range(0, x.shape[1], chunk)]
    return torch.cat([o for o, _ in parts], dim=1), torch.cat([j for _, j in parts], dim=1)


def _check(jac, what):
    if jac.dim() < 2:
        raise ValueError(f"{what} takes a Jacobian (..., O, dx), got shape {tuple(jac.shape)}")


def divergence(jac):
    """div u = sum_i d u_i / d x_i of a vector field with as many channels as coordinates: jac (..., O, dx), O == dx -> (...).
    Assumes CARTESIAN components: channel i is the field's component along coordinate i, and no metric factors are applied."""
    _check(jac, "divergence")
    if jac.shape[-2] != jac.shape[-1]:
        raise ValueError(f"divergence needs as many channels as coordinates, got (O, dx) = {tuple(jac.shape[-2:])}")
    return torch.diagonal(jac, dim1=-2, dim2=-1).sum(-1)


def curl_2d(jac):
    """The vorticity d v / d x - d u / d y of a 2-channel field (u, v) on 2 coordinates (x, y): jac (..., 2, 2) -> (...).
    Assumes CARTESIAN components: no metric factors are applied."""
    _check(jac, "curl_2d")
    if tuple(jac.shape[-2:]) != (2, 2):
        raise ValueError(f"curl_2d needs a 2-channel field on 2 coordinates, got (O, dx) = {tuple(jac.shape[-2:])}")
    return jac[..., 1, 0] - jac[..., 0, 1]


def gradient_norm(jac):
    """|grad u_o| per channel: jac (..., O, dx) -> (..., O), the Euclidean norm over the coordinates.
    Assumes CARTESIAN components: no metric factors are applied."""
    _check(jac, "gradient_norm")
    return jac.square().sum(-1).sqrt()
