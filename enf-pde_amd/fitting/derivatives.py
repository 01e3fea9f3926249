"""Derivative fields of a decoded signal: the Jacobian of the field w.r.t. the query coordinates from the native call
(EquivariantCrossAttentionNeF.jacobian, include/enf_hip.h: enf_field_grad) and the first-order operators built on it.

  decode_jacobian(...)   the counterpart of inner_loop.decode: (out, jac) on the full grid, chunking optional
  decode_tangent(...)    (out, tan) on the full grid: the decode in forward mode along a latent direction
                         (EquivariantCrossAttentionNeF.tangent, include/enf_hip.h: enf_field_tangent)
  decode_tendency(...)   (u, du/dt) on the full grid for latents that follow dz/dt = ode_model(z)
  decode_directional(...)          (u, D_c u = c . grad u) on the full grid along a direction field c in the query coordinates
  decode_material_derivative(...)  (u, Du/Dt = u_t + c . grad u): the latent ODE's tendency and the advection term in ONE tangent pass
  decode_second_directional(...)   (u, c . grad u, c^T H c): the second directional derivative in one second-order forward-mode pass
                                   (EquivariantCrossAttentionNeF.second_derivative, include/enf_hip.h: enf_field_second_x)
  decode_laplacian(...)            (u, grad u, lap u) from dx such passes along the unit vectors (Cartesian coordinates only)
  decode_hessian(...)              (u, grad u, hess u) from dx (dx + 1) / 2 passes, by polarisation
  decode_diffusion_residual(...)   (u, u_t - nu lap u) for latents that follow the latent ODE
  divergence / curl_2d / gradient_norm   operators on a Jacobian whose components are CARTESIAN

The Jacobian is w.r.t. the coordinates as the model takes them.  For the planar invariants these are Cartesian and the operators
below are the usual ones; for the spherical and ball invariants they are angles (and a radius), and a divergence or curl needs
the metric factors, which are not applied here.
"""
import torch

__all__ = ["decode_jacobian", "decode_tangent", "decode_tendency", "decode_directional", "decode_material_derivative", "divergence",
           "curl_2d", "gradient_norm", "decode_second_directional", "decode_laplacian", "decode_hessian", "decode_diffusion_residual"]


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


def decode_tangent(nef, nef_params, coords, p, a, window, dp, da, dwindow, chunk=None):
    """(out (B, N, O), tan (B, N, O)) on the full grid: tan = the directional derivative of the decode along the latent direction
    (dp, da, dwindow) -- shapes of p, a, window; ``None`` entries mean zero, not all three.  ``coords`` and ``chunk`` as in
    decode_jacobian: the chunks are slices of the grid, every query's result is the unchunked call's, bit for bit."""
    B = p.shape[0]
    x = coords[None].expand(B, -1, -1) if coords.dim() == 2 else coords
    if chunk is None:
        return nef.tangent(nef_params, x, p, a, window, dp=dp, da=da, dwindow=dwindow)
    parts = [nef.tangent(nef_params, x[:, i:i + chunk], p, a, window, dp=dp, da=da, dwindow=dwindow) for i in range(0, x.shape[1], chunk)]
    return torch.cat([o for o, _ in parts], dim=1), torch.cat([t for _, t in parts], dim=1)


def decode_tendency(nef, nef_params, ode_model, ode_params, coords, p, a, window, chunk=None):
    """(u (B, N, O), du/dt (B, N, O)) on the full grid for latents that follow the latent ODE: dz/dt = ode_model.apply(ode_params,
    (p, a, window)) is evaluated ONCE, without autograd, and pushed through the decoder by decode_tangent (du/dt = J_z dz/dt).
    ``None`` entries of the ODE's output mean zero (an ODE that leaves the window alone returns None or zeros for it)."""
    with torch.no_grad():
        dz = ode_model.apply(ode_params, (p, a, window))
    dp, da, dw = (None if v is None else v.detach().float().contiguous() for v in dz)
    if dw is not None:
        dw = dw.reshape(p.shape[0], p.shape[1], 1)
    return decode_tangent(nef, nef_params, coords, p, a, window, dp, da, dw, chunk=chunk)


def _tangent_x(nef, nef_params, coords, p, a, window, dp, da, dwindow, direction, chunk):
    """decode_tangent with a query direction beside the latent one: the chunks slice ``direction`` with the grid."""
    B = p.shape[0]
    x = coords[None].expand(B, -1, -1) if coords.dim() == 2 else coords
    xd = direction[None].expand(B, -1, -1) if direction.dim() == 2 else direction
    if tuple(xd.shape) != tuple(x.shape):
        raise ValueError(f"the direction has shape {tuple(direction.shape)}, expected (N, dx) or (B, N, dx) of the grid {tuple(x.shape)}")
    if chunk is None:
        return nef.tangent(nef_params, x, p, a, window, dp=dp, da=da, dwindow=dwindow, xdot=xd)
    parts = [nef.tangent(nef_params, x[:, i:i + chunk], p, a, window, dp=dp, da=da, dwindow=dwindow, xdot=xd[:, i:i + chunk])
             for i in range(0, x.shape[1], chunk)]
    return torch.cat([o for o, _ in parts], dim=1), torch.cat([t for _, t in parts], dim=1)


def decode_directional(nef, nef_params, coords, p, a, window, direction, chunk=None):
    """(u (B, N, O), D u (B, N, O)) on the full grid: D u[b, n, o] = sum_i d u[b, n, o] / d coords[n, i] direction[n, i], the derivative
    of the decoded field along ``direction`` -- an advection term c . grad u, the derivative along a streamline, a normal derivative on
    a boundary -- in one forward-mode pass (EquivariantCrossAttentionNeF.tangent with ``xdot``), no Jacobian formed.
    ``direction`` is (N, dx), one direction field for the batch, or (B, N, dx), float32, in COORDINATE RATES: the Jacobian's convention,
    coordinates as the model takes them.  On the sphere these are rates of the angles; a physical velocity is divided by its metric
    factors by the caller.  ``coords`` and ``chunk`` as in decode_jacobian: the chunks slice the direction with the grid, and every
    query's result is the unchunked call's, bit for bit."""
    return _tangent_x(nef, nef_params, coords, p, a, window, None, None, None, direction, chunk)


def decode_material_derivative(nef, nef_params, ode_model, ode_params, coords, p, a, window, velocity, chunk=None):
    """(u (B, N, O), Du/Dt (B, N, O)) on the full grid, Du/Dt = du/dt + velocity . grad u, for latents that follow the latent ODE:
    dz/dt = ode_model.apply(ode_params, (p, a, window)) is evaluated ONCE, without autograd, as in decode_tendency, and ONE tangent pass
    carries it together with the query direction ``velocity`` (forward mode is linear in its direction).
    ``velocity`` is (N, dx) or (B, N, dx), float32, in COORDINATE RATES as ``direction`` of decode_directional: on the sphere a physical
    velocity is divided by its metric factors by the caller.  ``None`` entries of the ODE's output mean zero.  ``chunk`` as in
    decode_directional."""
    with torch.no_grad():
        dz = ode_model.apply(ode_params, (p, a, window))
    dp, da, dw = (None if v is None else v.detach().float().contiguous() for v in dz)
    if dw is not None:
        dw = dw.reshape(p.shape[0], p.shape[1], 1)
    return _tangent_x(nef, nef_params, coords, p, a, window, dp, da, dw, velocity, chunk)


def _second_x(nef, nef_params, coords, p, a, window, direction, chunk, return_out=True):
    """(out or None, tan, tan2) of nef.second_derivative on the full grid; the chunks slice ``direction`` with the grid."""
    B = p.shape[0]
    x = coords[None].expand(B, -1, -1) if coords.dim() == 2 else coords
    xd = direction[None].expand(B, -1, -1) if direction.dim() == 2 else direction
    if tuple(xd.shape) != tuple(x.shape):
        raise ValueError(f"the direction has shape {tuple(direction.shape)}, expected (N, dx) or (B, N, dx) of the grid {tuple(x.shape)}")
    if chunk is None:
        return nef.second_derivative(nef_params, x, p, a, window, xd, return_out=return_out)
    parts = [nef.second_derivative(nef_params, x[:, i:i + chunk], p, a, window, xd[:, i:i + chunk], return_out=return_out)
             for i in range(0, x.shape[1], chunk)]
    return tuple(None if parts[0][k] is None else torch.cat([q[k] for q in parts], dim=1) for k in range(3))


def decode_second_directional(nef, nef_params, coords, p, a, window, direction, chunk=None):
    """(u (B, N, O), c . grad u (B, N, O), c^T H c (B, N, O)) on the full grid along a direction field c = ``direction`` in the query
    coordinates: the decode, its first and its second directional derivative, c^T H c = sum_ij c_i c_j d^2 u / d x_i d x_j, in one
    second-order forward-mode pass (EquivariantCrossAttentionNeF.second_derivative) -- a curvature along a streamline, a second normal
    derivative on a boundary.  ``direction``, ``coords`` and ``chunk`` as in decode_directional: coordinate rates, coordinates as the
    model takes them; every query's result is the unchunked call's, bit for bit.  Second derivatives as autograd means them: almost
    everywhere, the relu kinks contribute nothing."""
    return _second_x(nef, nef_params, coords, p, a, window, direction, chunk)


def _unit_passes(nef, nef_params, coords, p, a, window, chunk, pairs):
    """u, the first and second derivatives along the unit vectors e_i (lists of dx tensors), and with ``pairs`` the second derivatives
    along e_i + e_j, i < j (a dict): dx (+ dx (dx - 1) / 2) second-order passes, the decode stored by the first one only."""
    N, dx = coords.shape[-2], coords.shape[-1]

    def along(*axes):
        e = torch.zeros((N, dx), device=coords.device, dtype=torch.float32)
        e[:, list(axes)] = 1.0
        return e
    u, first, second, mixed = None, [], [], {}
    for i in range(dx):
        o, t, t2 = _second_x(nef, nef_params, coords, p, a, window, along(i), chunk, return_out=i == 0)
        u = o if i == 0 else u
        first.append(t)
        second.append(t2)
    if pairs:
        for i in range(dx):
            for j in range(i + 1, dx):
                mixed[(i, j)] = _second_x(nef, nef_params, coords, p, a, window, along(i, j), chunk, return_out=False)[2]
    return u, first, second, mixed


def decode_laplacian(nef, nef_params, coords, p, a, window, chunk=None):
    """(u (B, N, O), grad (B, N, O, dx), lap (B, N, O)) on the full grid: the decode, its gradient and its Laplacian
    lap = sum_i d^2 u / d x_i^2, from dx second-order forward-mode passes along the unit vectors (each returns a column of the gradient
    for free).  CARTESIAN coordinates only: for latitude_periodic / polar_periodic the coordinates are angles, a sum of second angle
    derivatives is not a physical operator and the call raises ValueError (metric-aware operators are not provided; decode_hessian
    gives the second derivatives in the coordinates as given).  ``coords`` and ``chunk`` as in decode_jacobian."""
    name = getattr(getattr(nef, "cross_attn_invariant", None), "name", None)
    if name in ("latitude_periodic", "polar_periodic"):
        raise ValueError(f"decode_laplacian: the coordinates of '{name}' are angles; a sum of second angle derivatives is not the "
                         "Laplacian on the sphere (metric-aware operators are out of scope: see decode_hessian)")
    u, first, second, _ = _unit_passes(nef, nef_params, coords, p, a, window, chunk, pairs=False)
    lap = second[0]
    for t2 in second[1:]:
        lap = lap + t2
    return u, torch.stack(first, dim=-1), lap


def decode_hessian(nef, nef_params, coords, p, a, window, chunk=None):
    """(u (B, N, O), grad (B, N, O, dx), hess (B, N, O, dx, dx)) on the full grid: hess[..., i, j] = d^2 u / d x_i d x_j in the
    coordinates as the model takes them (angles on the sphere, no metric factors), from dx second-order passes along the unit vectors
    and one per pair i < j along e_i + e_j, by polarisation: H_ij = (D2(e_i + e_j) - D2 e_i - D2 e_j) / 2.  Both triangles hold the
    same values: the result is symmetric bit for bit.  ``coords`` and ``chunk`` as in decode_jacobian."""
    u, first, second, mixed = _unit_passes(nef, nef_params, coords, p, a, window, chunk, pairs=True)
    dx = len(first)
    rows = [[None] * dx for _ in range(dx)]
    for i in range(dx):
        rows[i][i] = second[i]
        for j in range(i + 1, dx):
            rows[i][j] = rows[j][i] = (mixed[(i, j)] - second[i] - second[j]) * 0.5
    return u, torch.stack(first, dim=-1), torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def decode_diffusion_residual(nef, nef_params, ode_model, ode_params, coords, p, a, window, diffusivity, chunk=None):
    """(u (B, N, O), u_t - nu lap u (B, N, O)) on the full grid: the residual of the diffusion equation u_t = nu lap u for latents that
    follow the latent ODE -- u_t from decode_tendency (one first-order pass), lap u from decode_laplacian (dx second-order passes).
    ``diffusivity`` nu: a number, or a tensor that broadcasts against (B, N, O).  Cartesian coordinates, as decode_laplacian."""
    u, lap = decode_laplacian(nef, nef_params, coords, p, a, window, chunk=chunk)[::2]
    ut = decode_tendency(nef, nef_params, ode_model, ode_params, coords, p, a, window, chunk=chunk)[1]
    return u, ut - diffusivity * lap


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
