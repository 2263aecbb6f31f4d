"""Stock-torch restatement of an eval-mode GRU_RNN pass with hidden_layers >= 1 (reference gru_vae.py:322-455, live branch), in
fp64 by default: torch.nn.GRU(num_layers=L) stepped frame by frame with y_{t-1} = out_1(top-layer output) fed back, the two dilated
convolutions as F.conv1d.  For sizes too big to keep as goldens (the 64-row hu1024 pass); tests/test_stacked_cpu.py pins it to the
goldens recorded from the reference itself (tests/golden/stacked_*.npz).  Weights are a numpy state_dict with the reference's keys."""
import numpy as np
import torch
import torch.nn.functional as F

CLAMP_GAUSS = -13.815510557964274104107948728106      # ln(1e-6), gru_vae.py:412


def n_layers_of(sd):
    return 1 + max(int(k.rsplit("_l", 1)[1]) for k in sd if k.startswith("gru.weight_hh_l"))


def forward(sd, x, y_in, h_in=None, clamp_lat_dim=None, dtype=torch.float64):
    """x [B,T,Cin] (or [T,Cin]), y_in [B,1,Cout], h_in [L,B,H] or None -> (trj_out, y_last [B,1,Cout], h [L,B,H]) as numpy fp64."""
    w = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    two_d = x.ndim == 2
    xt = torch.from_numpy(np.asarray(x)).to(dtype)
    if two_d:
        xt = xt.unsqueeze(0)
    B, T, _ = xt.shape
    L = n_layers_of(sd)
    H = w["gru.weight_hh_l0"].shape[1]
    ks = w["conv.conv.0.weight"].shape[2]
    xin = xt.transpose(1, 2)
    if "scale_in.weight" in w:
        xin = F.conv1d(xin, w["scale_in.weight"], w["scale_in.bias"])
    c = F.conv1d(xin, w["conv.conv.0.weight"], w["conv.conv.0.bias"], padding=(ks * ks - 1) // 2)
    c = F.conv1d(c, w["conv.conv.1.weight"], w["conv.conv.1.bias"], dilation=ks)
    xconv = c.transpose(1, 2)                                   # [B, T, ks^2 * Cin]
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
        trj = torch.cat(trj, 1)
        if "scale_out.weight" in w:
            o = F.conv1d(trj.transpose(1, 2), w["scale_out.weight"], w["scale_out.bias"]).transpose(1, 2)
        else:
            o = trj
            if clamp_lat_dim is not None:
                o = torch.cat((o[:, :, :clamp_lat_dim], torch.clamp(o[:, :, clamp_lat_dim:], min=CLAMP_GAUSS)), 2)
    o = o.numpy()
    return (o[0] if two_d else o), y.numpy(), h.numpy()
