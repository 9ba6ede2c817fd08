"""What the SPFF-UNet GPU tests share (test infrastructure): a fixture's engine module, the
engine's own branch decisions, the kink-consistent fp64 / fp32 oracle gradients under them,
and the gradient bar.  The model-agnostic rules are tests/_compare.py."""
import numpy as np
import torch
import torch.nn.functional as F

from _compare import check_grads_rows, grad_errors
from _golden import build_core, cfg_of, state_of
from oracle import spff_oracle as O
import innovative3D.models as M

DEV = "cuda"


def load_core(d):
    meta = d["meta"]
    core = build_core(meta)
    D = d["x"].shape[2]
    for b in core._blocks():
        if isinstance(getattr(b, "fgate", None), M.FourierGate3D):
            b.fgate._ensure_mask(D, "cpu")
    st = state_of(d)
    core.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return core.to(DEV)


def synth_core(K, base, in_ch, D, seed, mask_jitter=0.0, **flags):
    """An SPFF-UNet (EnergyFiLM + FourierGate) on the host holding weightgen's synthetic state
    of ``seed``, its FourierGate masks sized for depth ``D``.  -> (core, that state)"""
    from innovative3D.weightgen import synth_state
    core = M.build_spct_energyfilm_fourier(num_classes=K, base=base, in_channels=in_ch, **flags)
    for b in core._blocks():
        b.fgate._ensure_mask(D, "cpu")
    st = synth_state([(k, tuple(v.shape)) for k, v in core.state_dict().items()], seed=seed,
                     mask_jitter=mask_jitter)
    core.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return core, st


def grad_scales(ref64, absb, st):
    """Per tensor: max over the tensor of sum_b |per-sample g_b| (absb); FourierGate mag_scale:
    at least the sum of its absolute terms."""
    scales = {}
    for kk in ref64:
        # scale: sum over samples of |per-sample gradient| (= max|g| for B=1); the batch
        # gradient is a sum of per-sample terms that can cancel (e.g. SE biases)
        scale = max(float(absb[kk].max()), 1e-12)
        if kk.endswith("fgate.mag_scale"):
            # d/d(mag) = sum_k mask_k dL/dM_k (M = mask * mag): a sum over the rfft
            # bins that can cancel almost completely; judge it against the sum of
            # its absolute terms, sum_k |mask_k dL/dM_k| = sum_k |mask_k g_mask_k| / |mag|
            pre = kk[: -len("mag_scale")]
            mk = pre + ("freq_mask" if pre + "freq_mask" in ref64 else "_mask")
            mag = abs(float(np.asarray(st[kk]).reshape(-1)[0]))
            terms = np.abs(np.asarray(st[pre + "freq_mask"]).reshape(-1) *
                           absb[mk].reshape(-1)).sum()
            scale = max(scale, float(terms) / max(mag, 1e-12))
        scales[kk] = scale
    return scales


def check_grads(grads, ref64, ref32, absb, st, mth):
    """Every engine gradient vs the kink-consistent fp64 oracle: max|g - g64| / scale
    within max(1e-3, 8 x the fp32 oracle's own error) (bf16x3: max(5e-3, 64 x); the
    floor alone when ``ref32`` is None); scale
    = max over the tensor of sum_b |per-sample g_b| (absb); FourierGate mag_scale is
    judged against the sum of its absolute terms."""
    floor, factor = (5e-3, 64) if mth == "bf16x3" else (1e-3, 8)
    rows = grad_errors(grads, ref64, ref32, scale=grad_scales(ref64, absb, st))
    check_grads_rows(rows, floor=floor, factor=factor, top=6)


def _block_names(cfg):
    a, b = ("pre", "body") if cfg.novel else ("b1", "b2")
    return [(blk, a, b) for blk in ("enc1", "enc2", "enc3", "bott", "dec3", "dec2", "dec1")]


def engine_branch_masks(core, xshape, st, cfg):
    """Sign pattern of every LeakyReLU input, and the argmax of every max-pool
    window, as the ENGINE saw them (the pools: from its saved pool inputs; ties
    resolved first-max like the engine and torch).  The LeakyReLUs: the engine's
    saved conv outputs y1/y2 under its own per-(b,c) affine (al, de).  A fp32 conv differs from the
    reference's by ~1e-6 relative, so an input sitting within that of the kink
    (|r| ~ 0) can take the other slope (1 vs 0.01) -- a legitimate fp32 outcome
    the reference could equally produce.  Feeding the engine's pattern to the
    oracle removes these knife-edge flips from the gradient comparison."""
    B = xshape[0]
    plan = core._plan
    masks = {}
    for blk, a, b in _block_names(cfg):
        for tag, key in ((a, "y1"), (b, "y2")):
            y = plan.saved(f"{blk}.{key}").double().cpu()
            C = y.shape[1]
            Dd = xshape[2]
            lvl = {"enc1": 0, "dec1": 0, "enc2": 1, "dec2": 1, "enc3": 2, "dec3": 2, "bott": 3}[blk]
            Hh_, Ww = xshape[3] >> lvl, xshape[4] >> lvl
            y = y.view(B, Dd, Hh_, Ww, C).permute(0, 4, 1, 2, 3)
            g = torch.from_numpy(st[f"{blk}.{tag}.1.weight"]).double()
            bb = torch.from_numpy(st[f"{blk}.{tag}.1.bias"]).double()
            m64 = F.instance_norm(y, weight=g, bias=bb, eps=1e-5) > 0
            # the engine's own fp32 normalisation r = fma(y, al, de): its sign is the
            # sign of the exact y*al + de, which fp64 reproduces
            j = "1" if key == "y1" else "2"
            al = plan.saved(f"{blk}.al{j}").double().cpu().reshape(B, C, 1, 1, 1)
            de = plan.saved(f"{blk}.de{j}").double().cpu().reshape(B, C, 1, 1, 1)
            # contiguous: this torch build's CPU instance_norm backward is wrong for a
            # channels-last-strided grad_output, which torch.where would propagate
            m = ((y * al + de) > 0).contiguous()
            nd = int((m != m64).sum())
            if nd:
                print(f"  {blk}.{tag}: {nd} knife-edge signs (engine affine vs fp64 IN)")
            masks[f"{blk}.{tag}"] = m
    # max-pool windows: the engine's own argmax bytes (k = 2 dh + dw, first max in scan
    # order), as its backward routed them -- also valid for lean plans, whose block
    # outputs live in backward scratch
    Dd = xshape[2]
    for k in range(3):
        Hh_, Ww = xshape[3] >> (k + 1), xshape[4] >> (k + 1)
        idx = plan.saved(f"pool{k + 1}.idx").to(torch.int64).cpu()
        C = idx.shape[1]
        masks[f"pool{k + 1}"] = idx.view(B, Dd, Hh_, Ww, C).permute(0, 4, 1, 2, 3).contiguous()
    return masks


def oracle_grads(d, masks):
    return oracle_grads_st(cfg_of(d["meta"]), state_of(d), d["x"], d["labels"], masks)


def oracle_grads_st(cfg, st, x, labels, masks, device="cpu", fp32=True):
    """fp64 and fp32 oracle parameter gradients (CPU; ``device`` evaluates the same
    restatement through PyTorch's fp64 device kernels, ``fp32=False`` skips the fp32
    run and returns None for it) whose LeakyReLUs take the
    given sign patterns; also returns how many entries differ from the fp64
    oracle's own pattern (knife-edge flips) and sum_b |g_b| (fp64 per-sample
    gradients with the global CE normalisation; sum_b g_b = g exactly since
    IN / SE / gates are per sample and the Dice term carries no gradient).
    ``x``, ``labels``: numpy arrays; ``st``: the state dict (numpy)."""
    st = {k: v for k, v in st.items() if not k.endswith("._mask")}
    d = {"x": np.ascontiguousarray(x), "labels": np.ascontiguousarray(labels)}
    out = []
    nflip = [0]
    orig, orig_pool = O.conv_in_lrelu, O.maxpool
    npool = [0]
    masks = {k: v.to(device) for k, v in masks.items()}

    def pool_hooked(t):
        k = npool[0] % 3
        npool[0] += 1
        idx = masks[f"pool{k + 1}"]
        B_, C_, D_, H_, W_ = t.shape
        v = t[..., :H_ // 2 * 2, :W_ // 2 * 2].reshape(B_, C_, D_, H_ // 2, 2, W_ // 2, 2)
        v = v.permute(0, 1, 2, 3, 5, 4, 6)
        v = v.reshape(B_, C_, D_, H_ // 2, W_ // 2, 4)
        if t.dtype == torch.float64:
            nflip[0] += int((v.detach().argmax(-1) != idx).sum())
        return v.gather(-1, idx.unsqueeze(-1)).squeeze(-1)

    def hooked(P_, pre, inp, ksd):
        y = F.conv3d(inp, P_[pre + ".0.weight"], None, padding=(ksd // 2, 1, 1))
        r = F.instance_norm(y, weight=P_[pre + ".1.weight"], bias=P_[pre + ".1.bias"], eps=1e-5)
        m = masks[pre]
        if r.dtype == torch.float64:
            nflip[0] += int((m != (r.detach() > 0)).sum())
        return torch.where(m, r, 0.01 * r)

    O.conv_in_lrelu = hooked
    O.maxpool = pool_hooked
    try:
        for dt in ((torch.float64, torch.float32) if fp32 else (torch.float64,)):
            P = O.params_from_state(st, dtype=dt, device=device)
            O.fwd_bwd(P, torch.from_numpy(d["x"]).to(device, dt),
                      torch.from_numpy(d["labels"]).to(device), cfg)
            out.append({k: v.grad.double().cpu().numpy() for k, v in P.items()})
            del P
        if not fp32:
            out.append(None)
        B = d["x"].shape[0]
        absb = {k: np.abs(v) for k, v in out[0].items()}
        if B > 1:
            yall = torch.from_numpy(d["labels"]).to(device)
            N = int((yall != 255).sum())
            full = dict(masks)
            absb = None
            for b in range(B):
                for k in full:
                    masks[k] = full[k][b:b + 1]
                P = O.params_from_state(st, dtype=torch.float64, device=device)
                lg = O.forward(P, torch.from_numpy(d["x"][b:b + 1]).to(device, torch.float64), cfg)
                (F.cross_entropy(lg, yall[b:b + 1], ignore_index=255, reduction="sum") / N).backward()
                gb = {k: np.abs(v.grad.cpu().numpy()) for k, v in P.items()}
                absb = gb if absb is None else {k: absb[k] + gb[k] for k in absb}
            for k in full:
                masks[k] = full[k]
            masks.update(full)
    finally:
        O.conv_in_lrelu, O.maxpool = orig, orig_pool
    return out[0], out[1], nflip[0], absb


def pack_masks(masks):
    """a rank's branch decisions, npz-ready: bool masks bit-packed, each with its shape"""
    mk = {}
    for kk, m in masks.items():
        a = m.numpy()
        mk["m_" + kk] = np.packbits(a) if a.dtype == np.bool_ else a.astype(np.uint8)
        mk["s_" + kk] = np.array(a.shape)
    return mk


def gather_masks(parts, axis):
    """the ranks' branch decisions concatenated along the sharded axis (2 = D, 3 = H)"""
    masks = {}
    for kk in (f[2:] for f in parts[0].files if f.startswith("m_")):
        segs = []
        for p in parts:
            shp = tuple(int(v) for v in p["s_" + kk])
            a = p["m_" + kk]
            a = np.unpackbits(a)[:int(np.prod(shp))].astype(bool) if kk[:4] != "pool" else a
            segs.append(a.reshape(shp))
        cat = np.concatenate(segs, axis=axis)
        masks[kk] = (torch.from_numpy(cat) if cat.dtype == np.bool_
                     else torch.from_numpy(cat.astype(np.int64)))
    return masks
