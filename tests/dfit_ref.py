"""GAILCost.update_disc (milo/milo/gail_cost.py:104-204) restated in closed form in torch on the
CPU, in fp64 (the yardstick) or fp32: the comparator of test_cpu_dfit.py / test_gpu_dfit.py and
tools/dfit_time.py at shapes the fixture g16_disc_update.npz does not hold.

The discriminator is x -> h0 = relu(x W0^T + b0) -> h1 = relu(h0 W1^T + b1) -> out = h1 w2^T + b2.
The gradient is that of  c e + (1 - c) m + lambda/2 mean_e |d out / d x|_2  (the regularizer
reg_coef sum 1/2 |W|^2 is detached by the reference: logged, no gradient).  With the ReLU masks
m0 = (h0_e > 0), m1 = (h1_e > 0), constants of the double backward:
  a1 = m1 * w2, a0 = m0 * (a1 W1), g = a0 W0 = d out / d x, U = lambda / (2 bs) g / |g| (0 where |g| = 0)
  gW0 += a0^T U, q0 = m0 * (U W0^T), gW1 += a1^T q0, gw2 += sum_rows m1 * (q0 W1^T); no bias terms.
"""
import numpy as np
import torch

NAMES = ("W0", "b0", "W1", "b1", "w2", "b2")
KEYS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")


# fixture G16 (tests/golden/make_golden_dfit.py): S = 29 (D = 58), hidden [160, 96] (padded to 256
# and 128: more than one tile), 300 expert rows, a replay buffer of max_size 200 filled by three
# adds of 500 rows in all (the ring wraps), three update_disc calls per block, then the chi^2
G16 = dict(S=29, hidden=[160, 96], n_expert=300, seed_expert=31, max_size=200, adds=[(200, 41), (180, 42), (120, 43)],
           steps=3, blocks={
               "sgd_ls": dict(loss="least_squares", opt="sgd", args={"lr": 0.00001, "momentum": 0.9}, seed=100,
                              mb_seeds=[51, 52, 53], bs=70),
               "adam_ll": dict(loss="log_likelihood", opt="adam", args={"lr": 1e-3}, seed=101, mb_seeds=None, bs=256)})
METRICS = ("expert_disc_loss", "model_based_disc_loss", "gradient_penalty", "regularizer_loss", "total_disc_loss")


def g16_inputs():
    """(expert rows [300, 58], the three (s, s') adds, the agent rows after them in logical order)."""
    S = G16["S"]
    expert = synthetic_rows(G16["n_expert"], S, G16["seed_expert"], 0.5, 0.3)
    adds = [synthetic_rows(n, S, seed, 0.7, -0.2) for n, seed in G16["adds"]]
    return expert, [(r[:, :S], r[:, S:]) for r in adds], torch.cat(adds, 0)[-G16["max_size"]:]


def g16_mb(cfg, k):
    """The agent batch passed to the k-th update_disc of a block (None: sampled from the buffer)."""
    return None if cfg["mb_seeds"] is None else synthetic_rows(cfg["bs"], G16["S"], cfg["mb_seeds"][k], 0.7, -0.2)


def synthetic_rows(n, S, seed, scale=0.5, shift=0.0):
    """Seeded float32 rows [n, 2 S] = [s, s'] with s' = s + a small step."""
    rs = np.random.RandomState(seed)
    s = scale * rs.randn(n, S) + shift
    s2 = s + 0.1 * rs.randn(n, S)
    return torch.from_numpy(np.concatenate([s, s2], 1)).float()


def init_weights(D, hidden, seed):
    """The six tensors GAILCost(seed=...) starts from (gail_cost.py:11-39, 62): torch.manual_seed,
    the Linear layers in order, then uniform(-1, 1) for the head and xavier_uniform for the rest."""
    torch.manual_seed(seed)
    sizes = [D] + list(hidden) + [1]
    layers = [torch.nn.Linear(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)]
    for lin in layers:
        if lin.out_features == 1:
            torch.nn.init.uniform_(lin.weight.data, a=-1.0, b=1.0)
        else:
            torch.nn.init.xavier_uniform_(lin.weight.data)
    return [t.data.clone() for lin in layers for t in (lin.weight, lin.bias)]


def forward(p, x):
    W0, b0, W1, b1, w2, b2 = p
    h0 = torch.relu(x @ W0.T + b0)
    h1 = torch.relu(h0 @ W1.T + b1)
    return h0, h1, h1 @ w2.T + b2


def losses_and_grads(p, x_e, x_m, loss_type, c, reg_coef, grad_lambda):
    """(metrics dict, gradients of the six tensors) of one update_disc batch."""
    W0, b0, W1, b1, w2, b2 = p
    bs = x_e.shape[0]
    x = torch.cat([x_e, x_m], 0)
    h0, h1, out = forward(p, x)
    oe, om = out[:bs], out[bs:]
    if loss_type == "least_squares":
        e, m = ((oe - 1.0) ** 2).mean(), ((om + 1.0) ** 2).mean()
        dout = torch.cat([2.0 * c * (oe - 1.0), 2.0 * (1.0 - c) * (om + 1.0)], 0) / bs
    else:
        se, sm = torch.sigmoid(oe), torch.sigmoid(om)
        e, m = -torch.log(se).mean(), -torch.log(1.0 - sm).mean()
        dout = torch.cat([-c * (1.0 - se), (1.0 - c) * sm], 0) / bs
    # the ordinary backward
    gw2, gb2 = dout.T @ h1, dout.sum(0)
    dz1 = (dout @ w2) * (h1 > 0)
    gW1, gb1 = dz1.T @ h0, dz1.sum(0)
    dz0 = (dz1 @ W1) * (h0 > 0)
    gW0, gb0 = dz0.T @ x, dz0.sum(0)
    # the gradient penalty over the expert rows
    m0, m1 = (h0[:bs] > 0).to(x.dtype), (h1[:bs] > 0).to(x.dtype)
    a1 = m1 * w2
    a0 = m0 * (a1 @ W1)
    g = a0 @ W0
    nrm = g.norm(dim=1, keepdim=True)
    U = torch.where(nrm > 0, (grad_lambda / (2.0 * bs)) * g / nrm.clamp_min(1e-300), torch.zeros_like(g))
    q0 = m0 * (U @ W0.T)
    gW0 = gW0 + a0.T @ U
    gW1 = gW1 + a1.T @ q0
    gw2 = gw2 + (m1 * (q0 @ W1.T)).sum(0, keepdim=True)
    pen = grad_lambda * 0.5 * nrm.mean()
    reg = reg_coef * sum(0.5 * (w ** 2).sum() for w in (W0, W1, w2))
    metrics = {"expert_disc_loss": float(e), "model_based_disc_loss": float(m), "gradient_penalty": float(pen),
               "regularizer_loss": float(reg), "total_disc_loss": float(c * e + (1.0 - c) * m + reg + pen)}
    if loss_type == "least_squares":
        metrics["expert_acc"] = float((oe > 0).to(x.dtype).mean())
        metrics["mb_acc"] = float((om < 0).to(x.dtype).mean())
    return metrics, [gW0, gb0, gW1, gb1, gw2, gb2]


def restate(weights, batches, loss_type, optim, lr, p1, c, reg_coef, grad_lambda, dtype, state=None):
    """`weights`: six tensors in NAMES' order (w2 [1, H1], b2 [1]); `batches`: [(x_e, x_m), ...].
    optim 'sgd' (p1 = momentum; torch.optim.SGD without Nesterov, dampening or weight decay) or
    'adam' (p1 = eps; betas 0.9 / 0.999).  `state`: None or dict(step, s1, s2) to resume.
    Returns dict(weights, state=dict(step, s1, s2), metrics=[...])."""
    p = [w.detach().clone().to(dtype) for w in weights]
    step = 0 if state is None else state["step"]
    s1, s2 = ([torch.zeros_like(w) for w in p] if state is None or state[k] is None else [v.to(dtype) for v in state[k]]
              for k in ("s1", "s2"))
    out = []
    for x_e, x_m in batches:
        met, grads = losses_and_grads(p, x_e.to(dtype), x_m.to(dtype), loss_type, c, reg_coef, grad_lambda)
        out.append(met)
        step += 1
        for i, g in enumerate(grads):
            g = g.reshape(p[i].shape)
            if optim == "sgd":
                s1[i] = s1[i] * p1 + g
                p[i] = p[i] - lr * s1[i]
            else:
                s1[i] = s1[i] + (g - s1[i]) * (1.0 - 0.9)
                s2[i] = s2[i] * 0.999 + (1.0 - 0.999) * g * g
                den = s2[i].sqrt() / np.sqrt(1.0 - 0.999 ** step) + p1
                p[i] = p[i] - (lr / (1.0 - 0.9 ** step)) * (s1[i] / den)
    return dict(weights=p, state=dict(step=step, s1=s1, s2=s2 if optim != "sgd" else None), metrics=out)


def chi2(weights, x_e, x_a, c, dtype):
    """compute_chi2_distance's value (gail_cost.py:221-228) for the given rows."""
    p = [w.to(dtype) for w in weights]
    oe, oa = forward(p, x_e.to(dtype))[2], forward(p, x_a.to(dtype))[2]
    return float(c * ((oe - 1.0) ** 2).mean() + (1.0 - c) * ((oa + 1.0) ** 2).mean())


def update_error(got, ref, init):
    """max |dW_got - dW_ref| / max |dW_ref| with dW = W - W_init: the error of the update."""
    got, ref, init = (torch.as_tensor(np.asarray(v)).double().reshape(-1) for v in (got, ref, init))
    return float(((got - init) - (ref - init)).abs().max() / (ref - init).abs().max())


def state_error(got, ref):
    got, ref = (torch.as_tensor(np.asarray(v)).double().reshape(-1) for v in (got, ref))
    return float((got - ref).abs().max() / ref.abs().max())
