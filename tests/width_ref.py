"""TEST INFRASTRUCTURE: the float64 references of the hidden-width tests (tests/test_width_cpu.py, tests/test_width_gpu.py).

  eval   frontend_ref.forward in float64 (tests/test_frontend_cpu.py pins it to goldens recorded from the reference; it steps
         torch.nn.GRU with any number of layers), run the way the drivers of tests/width_util.py run the library: one whole pass,
         two windows with the carried (y_last, h), a window with a y_in that is NOT out_1(h_in), one frame.
  train  oracle/torch_stock.train_forward with dtype=torch.float64: the same statements as the float32 checker, every tensor upcast
         (the zero state included), autograd for dx and the ten parameter gradients of sum(out * cot).

Each function returns plain float64 numpy arrays; the test modules build them once per module (a module-scoped cache) and never
write to them."""
import numpy as np
import torch

import frontend_ref as fref
from oracle import torch_stock as ts

Y_ODD = 0.37          # what is added to the carried y_last so that it is no longer out_1(h_in)


def eval_reference(sd, x, y_in, clamp_lat_dim, t_split):
    """{name: (trj, y_last [B,1,Co], h [L,B,H])} of the passes an eval case runs.  t_split: frames of the first window."""
    f = lambda *a, **k: fref.forward(sd, *a, clamp_lat_dim=clamp_lat_dim, **k)
    ref = {"whole": f(x, y_in)}
    ref["win0"] = f(x[:, :t_split], y_in)
    ref["win1"] = f(x[:, t_split:], ref["win0"][1], h_in=ref["win0"][2])
    ref["odd"] = f(x[:, t_split:], ref["win0"][1] + Y_ODD, h_in=ref["win0"][2])
    ref["one"] = f(x[:, :1], y_in)
    return ref


def train_reference(sd, x, y_in, h_in, cmask, gmask, cot, clamp_lat_dim):
    """dict(out, y_last [B,Co], h_last [B,H], dx, grads {state key: array}) of one train-mode pass and the backward of
    sum(out * cot), in float64."""
    out, y, h, P, xt = ts.train_forward(sd, x, y_in, h_in, cmask, gmask, clamp_lat_dim, dtype=torch.float64)
    (out * torch.from_numpy(np.asarray(cot)).to(torch.float64)).sum().backward()
    return {"out": out.detach().numpy(), "y_last": y.detach().numpy(), "h_last": h.detach().numpy(), "dx": xt.grad.numpy(),
            "grads": {k: v.grad.numpy() for k, v in P.items() if v.grad is not None}}
