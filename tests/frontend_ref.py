"""Stock-torch restatement of an eval-mode GRU_RNN pass whose conv front-end has ANY depth (reference gru_vae.py:39-66 and :322-455,
live branch), in fp64 by default: conv.0 zero-padded by (ks^layers - 1) / 2, conv.i with dilation ks^i, torch.nn.GRU stepped frame by
frame with y_{t-1} = out_1(h_{t-1}) fed back.  Written from the module's state dict alone: the depth is the number of conv.conv.i
keys, kernel_size the last axis of conv.conv.0.weight.  For row counts the reference is too slow to record goldens for;
tests/test_frontend_cpu.py pins it to the goldens recorded from the reference itself (tests/golden/frontend_*.npz)."""
import numpy as np
import torch
import torch.nn.functional as F

CLAMP_GAUSS = -13.815510557964274104107948728106      # ln(1e-6), gru_vae.py:412


def depth_of(sd):
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("conv.conv.") and k.endswith(".weight"))


def front_end(sd, x, dtype=torch.float64):
    """x [B,T,Cin] -> [B,T,ks^layers*Cin]: scale_in (when the state has one) and the conv stack, as TwoSidedDilConv1d.forward."""
    w = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items() if k.startswith(("scale_in.", "conv."))}
    layers, ks = depth_of(sd), w["conv.conv.0.weight"].shape[2]
    c = torch.from_numpy(np.asarray(x)).to(dtype).transpose(1, 2)
    if "scale_in.weight" in w:
        c = F.conv1d(c, w["scale_in.weight"], w["scale_in.bias"])
    for i in range(layers):
        c = F.conv1d(c, w["conv.conv.%d.weight" % i], w["conv.conv.%d.bias" % i], dilation=ks ** i,
                     padding=(ks ** layers - 1) // 2 if i == 0 else 0)
    return c.transpose(1, 2)


def forward(sd, x, y_in, h_in=None, clamp_lat_dim=None, dtype=torch.float64):
    """x [B,T,Cin] (or [T,Cin]), y_in [B,1,Cout], h_in [L,B,H] or None -> (trj_out, y_last [B,1,Cout], h [L,B,H]) as numpy."""
    w = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    two_d = np.asarray(x).ndim == 2
    x = np.asarray(x)[None] if two_d else np.asarray(x)
    B, T, _ = x.shape
    L = 1 + max(int(k.rsplit("_l", 1)[1]) for k in sd if k.startswith("gru.weight_hh_l"))
    H = w["gru.weight_hh_l0"].shape[1]
    xconv = front_end(sd, x, dtype)
    gru = torch.nn.GRU(xconv.shape[2] + w["out_1.weight"].shape[0], H, L, batch_first=True).to(dtype)
    gru.load_state_dict({k[4:]: v for k, v in w.items() if k.startswith("gru.")})
    gru.eval()
    y = torch.from_numpy(np.asarray(y_in)).to(dtype).reshape(B, 1, -1)
    h = torch.zeros(L, B, H, dtype=dtype) if h_in is None else torch.from_numpy(np.asarray(h_in)).to(dtype).reshape(L, B, H)
    trj = []
    with torch.no_grad():
        for t in range(T):
            out, h = gru(torch.cat((xconv[:, t:t + 1], y), 2), h)
            y = F.conv1d(out.transpose(1, 2), w["out_1.weight"], w["out_1.bias"]).transpose(1, 2)
            trj.append(y)
        o = torch.cat(trj, 1)
        if "scale_out.weight" in w:
            o = F.conv1d(o.transpose(1, 2), w["scale_out.weight"], w["scale_out.bias"]).transpose(1, 2)
        elif clamp_lat_dim is not None:
            o = torch.cat((o[:, :, :clamp_lat_dim], torch.clamp(o[:, :, clamp_lat_dim:], min=CLAMP_GAUSS)), 2)
    o = o.numpy()
    return (o[0] if two_d else o), y.numpy(), h.numpy()
