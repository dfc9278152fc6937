"""The reference's PPO update restated in torch on the CPU (the comparator of test_cpu_ppo.py,
test_gpu_ppo.py and tools/ppo_time.py): PPO.train_from_paths (mjrl/mjrl/algos/ppo_clip.py:58-103)
over the policy's tanh MLP with flat-order parameters (gaussian_mlp.py:36-62), torch.optim.Adam on
all seven tensors, injected index batches and the write-back's log_std clamp.  It runs in fp64
(the yardstick) or fp32 (the reference's own arithmetic).

The old policy has two forms (`old=`).  "snapshot": a fixed copy of the parameters the call
started from.  "tracks_mean": the old mean network IS the new one (MLP.set_param_values,
gaussian_mlp.py:75, 87, hands both views of one float32 buffer, so from the second call on Adam's
in-place steps move both) and only log_std keeps its old copy.  In fp32, snapshot for the first
call and tracks_mean from the second on reproduces the reference's parameters bit for bit (G20)."""
import numpy as np
import torch
import torch.nn.functional as F

from bcfit_ref import param_shapes, split_flat  # noqa: F401  (re-exported)

LOG_STD0 = -0.25


def mean_fp32(flat, S, A, obs):
    """The fp32 torch mean of the policy `flat` at float32(obs), as numpy float32."""
    W1, b1, W2, b2, W3, b3, _ = [torch.tensor(np.asarray(p, dtype=np.float32)) for p in split_flat(flat, S, A)]
    x = torch.from_numpy(np.asarray(obs)).float()
    with torch.no_grad():
        return F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, W1, b1)), W2, b2)), W3, b3).numpy()


def make_paths(lens, S, A, flat0, seed=5):
    """Seeded float64 paths (observations, advantages, rewards, then actions = the initial
    policy's fp32 mean + exp(-0.25) noise): G20's inputs (make_golden_ppo.py draws the same)."""
    rs = np.random.RandomState(seed)
    paths = []
    for l in lens:
        obs = rs.randn(l, S)
        adv = rs.randn(l) * 2 + 0.3
        rew = rs.randn(l)
        paths.append(dict(observations=obs, advantages=adv, rewards=rew))
    for p in paths:
        noise = rs.randn(len(p["observations"]), A)
        p["actions"] = np.float64(mean_fp32(flat0, S, A, p["observations"]) + np.exp(LOG_STD0) * noise)
    return paths


def concat(paths):
    return tuple(np.concatenate([p[k] for p in paths]) for k in ("observations", "actions", "advantages"))


def whiten(adv):
    adv = np.asarray(adv, dtype=np.float64)
    return (adv - np.mean(adv)) / (np.std(adv) + 1e-6)


class Host:
    """The policy's trainable_params and old_params as tensors of `dtype`, PPO's optimizer and
    one train_from_paths call per `update`."""

    def __init__(self, flat, S, A, dtype, lr=3e-4, clip_coef=0.2, min_log_std=-3.0):
        self.S, self.A, self.dtype, self.clip, self.min_log_std = S, A, dtype, clip_coef, min_log_std
        self.params = [torch.tensor(np.asarray(p, dtype=np.float32)).to(dtype).requires_grad_(True)
                       for p in split_flat(flat, S, A)]
        self.old = [p.detach().clone() for p in self.params]
        self.optimizer = torch.optim.Adam(self.params, lr=lr)

    def mean_LL(self, x, a, params):
        W1, b1, W2, b2, W3, b3, log_std = params
        mean = F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, W1, b1)), W2, b2)), W3, b3)
        zs = (a - mean) / torch.exp(log_std)
        LL = - 0.5 * torch.sum(zs ** 2, dim=1) + - torch.sum(log_std) + - 0.5 * self.A * np.log(2 * np.pi)
        return mean, LL

    def _old(self, tracks):
        return [p.detach() for p in self.params[:6]] + [self.old[6]] if tracks else self.old

    def surrogate_kl(self, x, a, adv, tracks):
        """(CPI_surrogate, kl_old_new) over all rows (batch_reinforce.py:41-56, gaussian_mlp.py:142-152)."""
        with torch.no_grad():
            old_mean, LL_old = self.mean_LL(x, a, self._old(tracks))
            new_mean, LL_new = self.mean_LL(x, a, self.params)
            surr = torch.mean(torch.exp(LL_new - LL_old) * adv)
            old_ls, new_ls = self._old(tracks)[6], self.params[6]
            old_std, new_std = torch.exp(old_ls), torch.exp(new_ls)
            Nr = (old_mean - new_mean) ** 2 + old_std ** 2 - new_std ** 2
            Dr = 2 * new_std ** 2 + 1e-8
            kl = torch.mean(torch.sum(Nr / Dr + new_ls - old_ls, dim=1))
        return surr.item(), kl.item()

    def update(self, obs, act, adv, batches, old="snapshot"):
        """One train_from_paths call on concatenated float64 arrays with `batches`
        [epochs][steps][64] in place of np.random.choice.  Returns a dict: adv_w (fp64, whitened),
        surr_before, surr_after, kl_dist, step_losses, step_clipped (rows with LR outside
        [1 - c, 1 + c]), margin (the nearest |LR - (1 -/+ c)| over all row uses), params_after (flat,
        before the clamp) and clamped (log_std entries the write-back clamps)."""
        tracks = {"snapshot": False, "tracks_mean": True}[old]
        adv_w = whiten(adv)
        x = torch.from_numpy(np.asarray(obs)).float().to(self.dtype)
        a = torch.from_numpy(np.asarray(act)).float().to(self.dtype)
        advt = torch.from_numpy(adv_w).float().to(self.dtype)
        surr_before, _ = self.surrogate_kl(x, a, advt, tracks)
        losses, clipped, margin = [], [], np.inf
        for idx in np.asarray(batches).reshape(-1, 64):
            i = torch.as_tensor(idx, dtype=torch.long)
            self.optimizer.zero_grad()
            with torch.no_grad():
                _, LL_old = self.mean_LL(x[i], a[i], self._old(tracks))
            _, LL_new = self.mean_LL(x[i], a[i], self.params)
            LR = torch.exp(LL_new - LL_old)
            LR_clip = torch.clamp(LR, min=1 - self.clip, max=1 + self.clip)
            loss = - torch.mean(torch.min(LR * advt[i], LR_clip * advt[i]))
            loss.backward()
            self.optimizer.step()
            lr = LR.detach().double().numpy()
            losses.append(loss.item())
            clipped.append(int((LR_clip != LR).sum()))
            margin = min(margin, float(np.min(np.minimum(np.abs(lr - (1 - self.clip)), np.abs(lr - (1 + self.clip))))))
        surr_after, kl = self.surrogate_kl(x, a, advt, tracks)
        after = self.flat()
        with torch.no_grad():  # set_param_values(params_after_opt, set_new=True, set_old=True)
            n_clamped = int((self.params[6] < self.min_log_std).sum())
            self.params[6].clamp_(min=self.min_log_std)
            self.old = [p.detach().clone() for p in self.params]
        return dict(adv_w=adv_w, surr_before=surr_before, surr_after=surr_after, kl_dist=kl,
                    step_losses=np.array(losses), step_clipped=np.array(clipped, dtype=np.int64), margin=margin,
                    params_after=after, clamped=n_clamped)

    def flat(self):
        return np.concatenate([p.detach().numpy().ravel() for p in self.params])

    def adam(self):
        """(step, [exp_avg], [exp_avg_sq]) over the seven tensors."""
        st = [self.optimizer.state[p] for p in self.params if p in self.optimizer.state]
        if not st:
            return 0, [], []
        return int(st[0]["step"]), [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st]
