"""The comparison rules of the GPU tests, once (test infrastructure; numpy only, importable
without a device; torch tensors and arrays are both accepted).

Logits: max|dlogit| within ``max_err`` of the reference and every argmax flip at a reference
near-tie (top-2 gap < 2 x the observed error), optionally at most ``max_flips`` of them.
Gradients: per tensor, max|g - g64| / scale within max(floor, factor x the fp32 oracle's own
error) of a kink-consistent fp64 oracle; a NaN or inf on either side fails.  Which floor,
factor, cap and scale each test module uses is tabulated in DESIGN.md ("Test strategy").
Every rejection is written ``not (x <= tol)``: ``x > tol`` lets a NaN pass."""
import hashlib
import math

import numpy as np


def _np(a, dtype=None):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype)


def near_tie_mask(ref_logits, tol):
    """[B, D, H, W] bool: the reference's top-2 gap along axis 1 is below ``tol``"""
    top2 = np.sort(_np(ref_logits), axis=1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) < tol


def check_logits(tag, lg, ref, *, max_flips=None, max_err=1e-3):
    """-> (err, number of argmax flips, flips).  The arithmetic is that of the dtypes given."""
    lg, ref = _np(lg), _np(ref)
    err = float(np.abs(lg - ref).max())
    flips = lg.argmax(1) != ref.argmax(1)
    nf = int(flips.sum())
    print(f"{tag}: max|dlogit| = {err:.3e}  argmax flips = {nf} of {flips.size}")
    assert err <= max_err, f"{tag}: max|dlogit| {err:.3e} above {max_err:.0e}"
    if nf:
        out = int((flips & ~near_tie_mask(ref, 2 * err)).sum())
        assert not out, f"{tag}: {out} of {nf} argmax flips outside near-ties"
    assert max_flips is None or nf <= max_flips, f"{tag}: {nf} argmax flips, at most {max_flips}"
    return err, nf, flips


def grad_errors(grads, ref64, ref32, *, scale=None):
    """rows (e_gpu, e_32, key), one per tensor of ``ref64``: max|g - g64| and max|g32 - g64|
    over ``scale[key]`` (default max(max|g64|, 1e-12)); ``ref32`` None: e_32 = 0."""
    rows = []
    for k, g64 in ref64.items():
        assert grads[k] is not None, k
        g64 = _np(g64, np.float64)
        s = scale[k] if scale is not None and k in scale else max(float(np.abs(g64).max()), 1e-12)
        e_gpu = float(np.abs(_np(grads[k], np.float64) - g64).max()) / s
        e_32 = float(np.abs(_np(ref32[k], np.float64) - g64).max()) / s if ref32 is not None else 0.0
        rows.append((e_gpu, e_32, k))
    return rows


def check_grads_rows(rows, *, floor=1e-3, factor=8, top=5, width=32):
    """Every row's e_gpu within max(floor, factor x e_32); a NaN or inf e_gpu fails, and so
    does an e_32 that is no number to set a bar by.  Prints the worst ``top`` rows."""
    bad = [f"{k}: gpu {a:.2e} vs fp32-oracle {b:.2e}" for a, b, k in rows
           if not (math.isfinite(b) and a <= max(floor, factor * b))]
    rows = sorted(rows, key=lambda r: (not r[0] <= math.inf, r), reverse=True)  # NaN first
    print("\n".join(f"  {k:{width}s} gpu {a:.2e}  fp32-oracle {b:.2e}" for a, b, k in rows[:top]))
    assert not bad, "; ".join(bad)


def ncdhw(t_cl, B, D, H, W):
    """engine channel-last [V, C] -> [B, C, D, H, W]"""
    return t_cl.view(B, D, H, W, -1).permute(0, 4, 1, 2, 3)


def kink_hooks(masks, pidx):
    """The kink-consistent oracles' hooks: ``relu`` keeps an input where the engine's output was
    positive (``masks[name]``, bool), ``pool`` takes the window entry the engine took
    (``pidx[name]``, max_pool3d indices).  -> (hooks, sha256 of all those decisions)."""
    h = hashlib.sha256()
    for k in sorted(masks):
        h.update(np.packbits(masks[k].numpy()).tobytes())
    for k in sorted(pidx):
        h.update(pidx[k].numpy().tobytes())

    def relu(name, r):
        return r * masks[name].to(r.dtype)

    def pool(name, v):
        idx = pidx[name]
        return v.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    return {"relu": relu, "pool": pool}, h.hexdigest()


def track_plan(m):
    """remember the plan the module used (its saved tensors feed the kink-consistent oracle)"""
    orig = m._plan

    def _plan(*args, _o=orig):
        p = _o(*args)
        m._last_plan = p
        return p
    m._plan = _plan


_ORACLE = {}


def cached_oracle(key, make):
    """``make()`` once per ``key`` ((fixture, branch digest): one oracle run per distinct set
    of branch decisions); the value is shared and left unchanged."""
    if key not in _ORACLE:
        _ORACLE[key] = make()
    return _ORACLE[key]


def assert_steps_bitwise(step):
    """``step()`` -> (logits, {name: gradient}), fresh tensors each call: two calls agree
    bitwise on the logits and on every gradient.  -> the first call's pair."""
    import torch
    (l1, g1), (l2, g2) = step(), step()
    assert torch.equal(l1, l2)
    assert g1.keys() == g2.keys()
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    return l1, g1


def assert_no_grad_forward_equals_train(m, x, *, eval_mode=False):
    """The no-grad forward (in eval mode where asked) returns the grad-mode forward's bits.
    -> the no-grad logits."""
    import torch
    a = m(x).detach().clone()
    if eval_mode:
        m.eval()
    with torch.no_grad():
        b = m(x)
    torch.cuda.synchronize()
    assert not b.requires_grad and torch.equal(a, b)
    return b


def lrelu_act_masks(plan, levels, B, D, H, W):
    """Sign patterns of residual blocks' LeakyReLU inputs as the engine saw them: sign(a1) and
    sign(out) (a LeakyReLU keeps the sign of its input).  ``levels``: block -> pooling level
    of its volume under [D, H, W]; -> {block.act1 / block.act2: bool [B, C, d, h, w]}."""
    out = {}
    for name, lvl in levels.items():
        for key, act in (("a1", "act1"), ("out", "act2")):
            t = ncdhw(plan.saved(f"{name}.{key}").cpu(), B, D >> lvl, H >> lvl, W >> lvl)
            out[f"{name}.{act}"] = (t > 0).contiguous()
    return out


def check_fixture_grads(d, grad_of):
    """A CPU oracle's fp32 gradients (``grad_of(name)`` -> array) against the ones a fixture
    stores, whole (``grad/``) or as head, tail and l2 norm (``gradhead/``, ``gradtail/``,
    ``gradsum/``): 5e-4 of max|ref| + 2e-5 of the largest gradient entry of the model (the
    fixture is one CPU's fp32 result, and another CPU's oneDNN sums in another order)."""
    gmax = max(float(np.abs(d[k]).max()) for k in d
               if k.startswith("grad/") or k.startswith("gradhead/"))
    for k in map(str, d["param_names"]):
        g = _np(grad_of(k))
        if "grad/" + k in d:
            ref_g = d["grad/" + k]
            scale = max(1e-6, float(np.abs(ref_g).max()))
            assert float(np.abs(g - ref_g).max()) <= 5e-4 * scale + 2e-5 * gmax, k
        else:
            flat = g.reshape(-1)
            scale = max(1e-6, float(np.abs(d["gradhead/" + k]).max()))
            np.testing.assert_allclose(flat[:64], d["gradhead/" + k], atol=5e-4 * scale + 2e-5 * gmax)
            np.testing.assert_allclose(flat[-64:], d["gradtail/" + k], atol=5e-4 * scale + 2e-5 * gmax)
            assert math.isclose(float(np.sqrt((flat.astype(np.float64) ** 2).sum())),
                                float(d["gradsum/" + k][1]), rel_tol=1e-4, abs_tol=1e-9), k


def fp32_bound(ref, cpu32):
    """The op tests' bar: 16 x the error the same fp32 computation in torch on the CPU shows
    against fp64, floored at 1e-6 of max|ref|.  -> (bound, that error, max|ref|)"""
    ref_max = float(ref.abs().max())
    e32 = float((cpu32.double() - ref).abs().max())
    return max(16.0 * e32, 1e-6 * ref_max), e32, ref_max
