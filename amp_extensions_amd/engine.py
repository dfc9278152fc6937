"""Device-resident building blocks over the amx C ABI: context, the dense-MLP ensemble,
RFF features and the reward kernels.

Layout in HBM (all fp32 unless noted; B_pad = round_up(B, 128)):
  act   [M][B_pad][ldk]     dense-concat activation rows: [s~, a~, 0-pad | h0 | h1 | h2 | h3]
                            (ldk = k0_pad + L*Hp; k0_pad = round_up(S+A, 32))
  W_i   [M][Hp][k0_pad+i*Hp] hidden-layer weights re-indexed into that column layout
  W_out [M][n_out_pad][ldk]  last layer, rows >= S zero
  preds [M][B_pad][S]        un-normalised state deltas of every member
Hidden widths that are not multiples of 128 are zero-padded (ReLU(0) = 0 keeps the pad
inert), so any BasicMLP config runs on the same 128x128 MFMA tiles.

A plain (dense_connect=False) context keeps those activation rows; only the weights differ:
  W_i   [M][Hp][Hp]          i >= 1: reads the K window [k0_pad + (i-1)*Hp, k0_pad + i*Hp)
  W_out [M][n_out_pad][Hp]   reads the last hidden window
(W_0 [M][Hp][k0_pad] as above; DeviceEnsemble.layer_windows).
"""
from __future__ import annotations


import numpy as np
import torch

from . import _native as N
from .humanoid import TerminationConfig
from .optstate import ensemble_layout, pack_state, plain_ensemble_layout


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class AmxContext:
    """One amx_ctx per device (include/amx_hip.h)."""

    def __init__(self, S: int, A: int, n_models: int = 4, hidden: int = 512, n_hidden: int = 4,
                 feat_dim: int = 512, device: torch.device | str | int = "cuda", dense_connect: bool = True):
        """dense_connect=False: a plain BasicMLP (amx_create_ex with AMX_CONNECT_PLAIN)."""
        self.lib = N.load()
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if self.device.type != "cuda":
            raise N.AmxNativeError("the amx engine runs on a ROCm GPU only (no CPU path)")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.S, self.A, self.M = S, A, n_models
        self.Hp = round_up(hidden, 128)
        self.L = n_hidden
        self.F = round_up(feat_dim, 128)
        self.dense_connect = bool(dense_connect)
        with torch.cuda.device(idx):
            if self.dense_connect:
                h = self.lib.amx_create(idx, S, A, n_models, self.Hp, n_hidden, self.F)
            else:
                h = self.lib.amx_create_ex(idx, S, A, n_models, self.Hp, n_hidden, self.F, N.AMX_CONNECT_PLAIN)
        if not h:
            raise N.AmxNativeError("amx_create failed: " + self.lib.amx_last_error().decode())
        self.h = h
        # device buffers registered with the context (split-K workspaces, timers): captured HIP
        # graphs bake their pointers into kernel arguments, so none is ever freed before the context
        self._retained = []
        k0, ldk, nout, kr = (N.C.c_int(), N.C.c_int(), N.C.c_int(), N.C.c_int())
        N.check(self.lib.amx_layout(h, N.C.byref(k0), N.C.byref(ldk), N.C.byref(nout), N.C.byref(kr)), "amx_layout")
        self.k0_pad, self.ldk, self.n_out_pad, self.k_rff_pad = k0.value, ldk.value, nout.value, kr.value
        # compute units (the C side's tile choices use the same device property)
        self.n_cus = torch.cuda.get_device_properties(self.device).multi_processor_count

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.amx_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def gemm_timer(self, on: bool = True):
        """In-kernel timing of the f16x3 ensemble forwards (amx_set_gemm_timer): returns the
        device buffer [start, arrivals, ticks (100 MHz), forwards], zeroed; off with on=False."""
        if not on:
            N.check(self.lib.amx_set_gemm_timer(self.h, None), "amx_set_gemm_timer")
            return None
        self._timer = torch.zeros(4, dtype=torch.int64, device=self.device)
        # graphs captured while an earlier timer was registered keep writing to it: every
        # buffer ever handed to the context lives as long as the context
        self._retained.append(self._timer)
        N.check(self.lib.amx_set_gemm_timer(self.h, self._timer.data_ptr()), "amx_set_gemm_timer")
        return self._timer

    @property
    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def set_normalizers(self, norms) -> None:
        arrs = [np.ascontiguousarray(torch.as_tensor(x).detach().cpu().float().numpy()) for x in norms]
        assert arrs[0].shape == (self.S,) and arrs[2].shape == (self.A,) and arrs[4].shape == (self.S,)
        self._norm_host = arrs  # keep alive during the (synchronous) copy
        N.check(self.lib.amx_set_normalizers(self.h, *[a.ctypes.data for a in arrs]), "amx_set_normalizers")

    def set_termination(self, cfg: TerminationConfig) -> None:
        ids, shapes, p0, p1 = cfg.tables()
        ids_a = np.ascontiguousarray(ids, dtype=np.int32)
        sh_a = np.ascontiguousarray(shapes, dtype=np.int32)
        p0_a = np.ascontiguousarray(p0, dtype=np.float64)
        p1_a = np.ascontiguousarray(p1, dtype=np.float64)
        N.check(self.lib.amx_set_termination(
            self.h, len(ids), ids_a.ctypes.data, sh_a.ctypes.data, p0_a.ctypes.data, p1_a.ctypes.data,
            int(cfg.record_all_world), int(cfg.record_world_root_pos), cfg.pos_dim, cfg.rot_dim, int(cfg.horizon),
            int(cfg.enable_velocity_check), int(cfg.vel_offset), float(cfg.vel_threshold),
            int(cfg.record_vel_as_pos), float(cfg.sampling_rate)), "amx_set_termination")

    # ---- thin checked launchers -------------------------------------------------------
    def gemm_bias_act(self, groups, rows, Nn, K, A, lda, sA, W, ldw, sW, bias, sB, C, ldc, sC, col_off, act):
        N.check(self.lib.amx_gemm_bias_act(self.h, groups, rows, Nn, K, A.data_ptr(), lda, sA, W.data_ptr(), ldw, sW,
                                           bias.data_ptr(), sB, C.data_ptr(), ldc, sC, col_off, act, self.stream),
                "amx_gemm_bias_act")


def split_bf16x3(ctx: AmxContext, W: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """3-limb bf16 image [G][rows][K/16][3][16] (int16 bits) of a [G][rows][K] fp32 device
    weight (amx_split_bf16x3), the operand of the amx_*_x6 GEMMs; `out` rewrites an image in place."""
    G, rows, K = W.shape
    W = W.contiguous()
    W3 = torch.empty(G, rows, 3 * K, dtype=torch.int16, device=ctx.device) if out is None else out
    _check_dev(W3, torch.int16, "out", ctx.device)
    if tuple(W3.shape) != (G, rows, 3 * K):
        raise ValueError(f"out: expected shape {(G, rows, 3 * K)}, got {tuple(W3.shape)}")
    N.check(ctx.lib.amx_split_bf16x3(ctx.h, G, rows, K, W.data_ptr(), K, rows * K, W3.data_ptr(), rows * 3 * K,
                                     ctx.stream), "amx_split_bf16x3")
    return W3


def split_f16x2(ctx: AmxContext, W: torch.Tensor, out=None):
    """Scaled 2-limb fp16 image [G][rows][K/16][2][16] (int16 bits) + row exponents [G][rows]
    of a [G][rows][K] fp32 device weight (amx_split_f16x2), the operand of the amx_*_h3 GEMMs;
    `out` = (image, exponents) rewrites an existing pair in place."""
    G, rows, K = W.shape
    W = W.contiguous()
    if out is None:
        W2 = torch.empty(G, rows, 2 * K, dtype=torch.int16, device=ctx.device)
        wexp = torch.empty(G, rows, dtype=torch.int32, device=ctx.device)
    else:
        W2, wexp = out
        _check_dev(W2, torch.int16, "out[0]", ctx.device)
        _check_dev(wexp, torch.int32, "out[1]", ctx.device)
        if tuple(W2.shape) != (G, rows, 2 * K) or tuple(wexp.shape) != (G, rows):
            raise ValueError(f"out: expected shapes {(G, rows, 2 * K)} and {(G, rows)}, got "
                             f"{tuple(W2.shape)} and {tuple(wexp.shape)}")
    N.check(ctx.lib.amx_split_f16x2(ctx.h, G, rows, K, W.data_ptr(), K, rows * K, W2.data_ptr(), rows * 2 * K,
                                    wexp.data_ptr(), rows, ctx.stream), "amx_split_f16x2")
    return W2, wexp


def flat_pairs(pairs, L: int):
    """[(W, b), ...] of L + 1 layers -> [W0, b0, W1, ...] (torch's parameter order); None: no tensors."""
    return [t for Wb in pairs or [(None, None)] * (L + 1) for t in Wb]


def _check_dev(t: torch.Tensor, dtype, name: str, device) -> None:
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor on {device}, got "
                         f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')}")


class DeviceEnsemble:
    """The BasicMLP ensemble resident in HBM (milo/milo/dynamics.py:19-233), dense-connect or
    plain as its context is (AmxContext.dense_connect).

    `weights[m]` = [(W0, b0), ..., (WL, bL)] in nn.Linear layout (W [out, in]); `norms` =
    the 6 transformation vectors of AmpDataset.get_transformations (datasets.py:23-43).
    All members share the normalizers (DynamicsEnsemble.load_ensemble, dynamics.py:128-131).
    """

    GEMM_PRECISIONS = ("f16x3", "bf16x6", "f32")

    def __init__(self, ctx: AmxContext, weights, norms, threshold: float = 0.0, gemm: str = "f16x3"):
        """gemm: "bf16x6" (fp32 operands split into 3 bf16 limbs, 6 limb products on the bf16
        MFMA pipe: fp32-level error, amx_gemm_*_x6), "f16x3" (power-of-two scaled operands
        split into 2 fp16 limbs, 3 products; the default) or "f32" (v_mfma_f32_32x32x2_f32)."""
        if gemm not in self.GEMM_PRECISIONS:
            raise ValueError(f"gemm must be one of {self.GEMM_PRECISIONS}, got {gemm!r}")
        self.gemm = gemm
        # exponent slots per row (f16x3): x0, h0 .. h_{L-1}
        self.n_slots = ctx.L + 1
        self.shared_x0 = True  # f16x3: x0 assembled once, read by every member (k_shared)
        self.ctx = ctx
        M, Hp, L = ctx.M, ctx.Hp, ctx.L
        if len(weights) != M:
            raise ValueError(f"expected {M} ensemble members, got {len(weights)}")
        hidden = weights[0][0][0].shape[0]
        self.hidden = hidden
        if round_up(hidden, 128) != Hp or len(weights[0]) != L + 1:
            raise ValueError("weights do not match the context's (hidden, n_hidden)")
        self.plain = not ctx.dense_connect
        if self.plain:
            if L < 1:
                raise ValueError("a plain ensemble needs at least one hidden layer")
            self.layout = plain_ensemble_layout(ctx.S, ctx.A, hidden, L, ctx.k0_pad, Hp, ctx.n_out_pad)
        else:
            self.layout = ensemble_layout(ctx.S, ctx.A, hidden, L, ctx.k0_pad, Hp, ctx.ldk, ctx.n_out_pad)  # per member
        self.W = self.b = self.W3 = self.W2 = self.wexp = None
        self.set_weights(weights)
        ctx.set_normalizers(norms)
        self.norms = tuple(torch.as_tensor(x).float().to(ctx.device) for x in norms)
        self.threshold = float(threshold)
        self._ws = {}
        # optional timing hook: when a list, every forward appends a (start, end) pair of
        # torch.cuda.Events recorded on the launch stream around the L+1 GEMM launches (inside
        # captured graphs use the context's in-kernel timer instead: AmxContext.gemm_timer)
        self.gemm_events = None

    def set_weights(self, weights) -> None:
        """(Re)load the members' nn.Linear weights, re-indexed into the dense-concat column
        layout and split into the GEMM path's limb image.  After the first call the device
        buffers are updated in place, so engines and captured graphs that hold their pointers
        see the new weights (DynamicsEnsemble.load_ensemble, dynamics.py:118-131)."""
        ctx = self.ctx
        M, L, dev = ctx.M, ctx.L, ctx.device
        if len(weights) != M:
            raise ValueError(f"expected {M} ensemble members, got {len(weights)}")
        rows = []
        for m, w in enumerate(weights):
            if len(w) != L + 1:
                raise ValueError(f"member {m}: {len(w)} layers, expected {L + 1}")
            try:
                rows.append(self.layout.pack([t for Wb in w for t in Wb]))
            except ValueError as e:
                raise ValueError(f"member {m}: {e}") from None
        padded = self.layout.views(torch.stack(rows))
        Ws, bs = padded[0::2], padded[1::2]
        if self.W is None:
            self.W = [w.to(dev).contiguous() for w in Ws]
            self.b = [b.to(dev).contiguous() for b in bs]
            if self.gemm == "bf16x6":
                self.W3 = [split_bf16x3(ctx, W) for W in self.W]
            elif self.gemm == "f16x3":
                sp = [split_f16x2(ctx, W) for W in self.W]
                self.W2, self.wexp = [x[0] for x in sp], [x[1] for x in sp]
            return
        for i in range(L + 1):
            self.W[i].copy_(Ws[i])
            self.b[i].copy_(bs[i])
            if self.W3 is not None:
                split_bf16x3(ctx, self.W[i], out=self.W3[i])
            if self.W2 is not None:
                split_f16x2(ctx, self.W[i], out=(self.W2[i], self.wexp[i]))

    @property
    def num_models(self) -> int:
        return self.ctx.M

    def layer_windows(self):
        """(first column, K) of the activation row that layer i = 0 .. L reads: the leading
        k0_pad + i*Hp columns (the whole row for the output layer) of a dense-connect net, the
        previous layer's Hp columns of a plain one."""
        c = self.ctx
        if not self.plain:
            return [(0, c.k0_pad + i * c.Hp) for i in range(c.L + 1)]
        return [(0, c.k0_pad)] + [(c.k0_pad + (i - 1) * c.Hp, c.Hp) for i in range(1, c.L + 1)]

    def workspace(self, B: int):
        """Activation + prediction buffers for B lanes (cached per B_pad).  B_pad = round_up(B, 128),
        or to 256 for large odd counts (the relabel's 40 530 samples: the 256 x 256 tiles need it)."""
        Bp = round_up(max(B, 1), 128)
        if Bp >= 16384 and Bp % 256:
            Bp += 128
        ws = self._ws.get(Bp)
        if ws is None:
            c = self.ctx
            ws = dict(Bp=Bp, act=torch.zeros(c.M, Bp, c.ldk, dtype=torch.float32, device=c.device),
                      preds=torch.zeros(c.M, Bp, c.S, dtype=torch.float32, device=c.device),
                      # f16x3: row exponents [M][slots][Bp] (x0, h0..h_{L-1})
                      rexp=torch.zeros(c.M, self.n_slots, Bp, dtype=torch.int32, device=c.device))
            if self.W2 is not None:
                self._ensure_split_workspace(Bp)
            self._ws[Bp] = ws
        return ws

    def workspace_blocked(self, Bq: int):
        """Buffers of the member-blocked forward (forward_blocked): M blocks of Bq lanes, lane
        b = g * Bq + r runs member g only.  act [1][M * Bq][ldk] (one x0 per lane), preds
        [M * Bq][S] (lane b's delta at row b), row exponents [M][slots][Bq] (the member-blocked
        exponent layout of amx_assemble_input_rexp / amx_policy_act: slot stride Bq)."""
        if Bq <= 0 or Bq % 128:
            raise ValueError(f"member blocks of {Bq} lanes: must be a positive multiple of 128")
        key = ("blocked", Bq)
        ws = self._ws.get(key)
        if ws is None:
            c = self.ctx
            ws = dict(Bq=Bq, act=torch.zeros(1, c.M * Bq, c.ldk, dtype=torch.float32, device=c.device),
                      preds=torch.zeros(c.M * Bq, c.S, dtype=torch.float32, device=c.device),
                      rexp=torch.zeros(c.M, self.n_slots, Bq, dtype=torch.int32, device=c.device))
            self._ensure_split_workspace(Bq)
            self._ws[key] = ws
        return ws

    def forward_blocked(self, ob: torch.Tensor, act: torch.Tensor, Bq: int, x0_ready: bool = False) -> torch.Tensor:
        """One member per lane: lanes [g * Bq, (g + 1) * Bq) through member g alone (SimEnv.step
        runs the lane's current member only, sim_env.py:154-157, with reset_counter % M choosing
        it at reset, :282-283).  A quarter of forward_preds' rows for the reference-semantics
        sampler, whose lanes are placed in the block of their trajectory's member.  Returns
        preds [M * Bq][S] (view of the workspace).  f16x3 only.  `x0_ready`: the policy launch
        already wrote x0 and its exponents into workspace_blocked(Bq) (amx_policy_act's fused
        assembly in the member-blocked layout)."""
        if self.W2 is None:
            raise ValueError("forward_blocked needs the f16x3 GEMM")
        c = self.ctx
        B = c.M * Bq
        if ob.dtype != act.dtype or ob.dtype not in (torch.float64, torch.float32):
            raise ValueError("ob and act must both be float64 or both float32")
        _check_dev(ob, ob.dtype, "ob", c.device)
        _check_dev(act, act.dtype, "act", c.device)
        if ob.shape[-1] != c.S or act.shape[-1] != c.A or ob.shape[0] < B or act.shape[0] < B:
            raise ValueError(f"ob {tuple(ob.shape)} / act {tuple(act.shape)} do not match S={c.S}, A={c.A}, "
                             f"{c.M} blocks of {Bq} lanes")
        ws = self.workspace_blocked(Bq)
        buf, preds, rexp = ws["act"], ws["preds"], ws["rexp"]
        s = c.stream
        dt = N.AMX_IN_F64 if ob.dtype == torch.float64 else N.AMX_IN_F32
        sA, sR, L = Bq * c.ldk, self.n_slots * Bq, c.L
        if not x0_ready:  # x0 once per lane + slot 0 of its member block's exponents (slot stride Bq)
            N.check(c.lib.amx_assemble_input_rexp(c.h, ob.data_ptr(), act.data_ptr(), dt, buf.data_ptr(), 0, c.ldk, B,
                                                  rexp.data_ptr(), sR, Bq, self.n_slots, s), "amx_assemble_input_rexp")
        if self.plain:
            self._mlp_h3_plain(buf, preds, Bq, s, rexp, sA, sR, Bq * c.S, 0)
            return preds
        for i in range(L):
            K = c.k0_pad + i * c.Hp
            N.check(c.lib.amx_gemm_bias_act_h3(c.h, c.M, Bq, c.Hp, K, buf.data_ptr(), c.ldk, sA, self.W2[i].data_ptr(),
                                               c.Hp * 2 * K, self.wexp[i].data_ptr(), c.Hp, self.b[i].data_ptr(), c.Hp,
                                               buf.data_ptr(), c.ldk, sA, K, N.AMX_ACT_RELU, rexp.data_ptr(), sR,
                                               i + 1, rexp[0, i + 1].data_ptr(), 0, s), "amx_gemm_bias_act_h3")
        N.check(c.lib.amx_gemm_out_unnorm_h3(c.h, c.M, Bq, c.S, c.ldk, buf.data_ptr(), c.ldk, sA,
                                             self.W2[L].data_ptr(), c.n_out_pad * 2 * c.ldk, self.wexp[L].data_ptr(),
                                             c.n_out_pad, self.b[L].data_ptr(), c.n_out_pad, preds.data_ptr(), c.S,
                                             Bq * c.S, rexp.data_ptr(), sR, L + 1, 0, s), "amx_gemm_out_unnorm_h3")
        return preds

    def _mlp_h3_plain(self, buf, preds, rows, s, rexp, sA, sR, sP, k_shared):
        """The f16x3 forward of a plain net over `rows` rows per member: layer 0 as the dense
        one's (x0, slot 0, shared below k_shared), then each layer on the window and the one
        exponent slot of the layer before it (amx_gemm_*_h3_win)."""
        c = self.ctx
        L, Hp, k0 = c.L, c.Hp, c.k0_pad
        N.check(c.lib.amx_gemm_bias_act_h3(c.h, c.M, rows, Hp, k0, buf.data_ptr(), c.ldk, sA, self.W2[0].data_ptr(),
                                           Hp * 2 * k0, self.wexp[0].data_ptr(), Hp, self.b[0].data_ptr(), Hp,
                                           buf.data_ptr(), c.ldk, sA, k0, N.AMX_ACT_RELU, rexp.data_ptr(), sR, 1,
                                           rexp[0, 1].data_ptr(), k_shared, s), "amx_gemm_bias_act_h3")
        for i in range(1, L):
            a0 = buf.data_ptr() + 4 * (k0 + (i - 1) * Hp)
            N.check(c.lib.amx_gemm_bias_act_h3_win(c.h, c.M, rows, Hp, Hp, a0, c.ldk, sA, self.W2[i].data_ptr(),
                                                   Hp * 2 * Hp, self.wexp[i].data_ptr(), Hp, self.b[i].data_ptr(), Hp,
                                                   buf.data_ptr(), c.ldk, sA, k0 + i * Hp, N.AMX_ACT_RELU,
                                                   rexp.data_ptr(), sR, i, rexp[0, i + 1].data_ptr(), 0, s),
                    "amx_gemm_bias_act_h3_win")
        a0 = buf.data_ptr() + 4 * (k0 + (L - 1) * Hp)
        N.check(c.lib.amx_gemm_out_unnorm_h3_win(c.h, c.M, rows, c.S, Hp, a0, c.ldk, sA, self.W2[L].data_ptr(),
                                                 c.n_out_pad * 2 * Hp, self.wexp[L].data_ptr(), c.n_out_pad,
                                                 self.b[L].data_ptr(), c.n_out_pad, preds.data_ptr(), c.S, sP,
                                                 rexp.data_ptr(), sR, L, s), "amx_gemm_out_unnorm_h3_win")

    def _ensure_split_workspace(self, Bp: int) -> None:
        """Register the output layer's split-K scratch with the context when Bp lanes split
        (amx_split_workspace_floats > 0); the buffer only grows.  A replaced buffer stays
        alive (AmxContext._retained): graphs captured before the growth still launch with its
        pointers, and its self-resetting arrival counters are zero between launches."""
        c = self.ctx
        nc = N.C.c_int(0)
        floats = int(c.lib.amx_split_workspace_floats(c.h, c.M, Bp, N.C.byref(nc)))
        if floats <= 0:
            return
        cur = getattr(c, "_split_ws", None)
        if cur is not None and cur[0].numel() >= floats and cur[1].numel() >= nc.value:
            return
        scratch = torch.empty(floats, dtype=torch.float32, device=c.device)
        counters = torch.zeros(max(nc.value, 1), dtype=torch.int32, device=c.device)
        N.check(c.lib.amx_set_split_workspace(c.h, scratch.data_ptr(), floats, counters.data_ptr(), nc.value),
                "amx_set_split_workspace")
        c._split_ws = (scratch, counters)
        c._retained.append(c._split_ws)

    def forward_preds(self, ob: torch.Tensor, act: torch.Tensor, B: int | None = None,
                      assembled: bool = False, x0_ready: bool = False) -> torch.Tensor:
        """All members' un-normalised deltas for rows [0, B): returns preds [M, Bp, S] (view
        of the workspace; rows >= B are padding).  ob/act fp64 or fp32 on the device.
        `x0_ready` (f16x3): the caller (amx_policy_act's fused assembly) already wrote the shared
        x0 slice into model 0's rows and the row-exponent slots of the workspace."""
        c = self.ctx
        B = ob.shape[0] if B is None else B
        if ob.dtype != act.dtype or ob.dtype not in (torch.float64, torch.float32):
            raise ValueError("ob and act must both be float64 or both float32")
        _check_dev(ob, ob.dtype, "ob", c.device)
        _check_dev(act, act.dtype, "act", c.device)
        if ob.shape[-1] != c.S or act.shape[-1] != c.A or ob.shape[0] < B or act.shape[0] < B:
            raise ValueError(f"ob {tuple(ob.shape)} / act {tuple(act.shape)} do not match S={c.S}, A={c.A}, B={B}")
        ws = self.workspace(B)
        Bp, buf, preds = ws["Bp"], ws["act"], ws["preds"]
        dt = N.AMX_IN_F64 if ob.dtype == torch.float64 else N.AMX_IN_F32
        s = c.stream
        rexp = ws["rexp"]
        k_shared = 0
        if x0_ready:
            if self.W2 is None:
                raise ValueError("x0_ready needs the f16x3 GEMM (shared x0 slice + row exponents)")
            self._mlp(buf, preds, Bp, s, rexp, row_exponents=False, k_shared=c.k0_pad)
            return preds
        if not assembled and self.W2 is not None:  # x0 + its row exponents in one pass
            # shared_x0: one x0 copy (model 0's rows) that every model's GEMMs read (k_shared)
            k_shared = c.k0_pad if self.shared_x0 else 0
            N.check(c.lib.amx_assemble_input_rexp(c.h, ob.data_ptr(), act.data_ptr(), dt, buf.data_ptr(),
                                                  0 if k_shared else Bp * c.ldk, c.ldk, B, rexp.data_ptr(),
                                                  (c.L + 1) * Bp, Bp, c.L + 1, s), "amx_assemble_input_rexp")
        elif not assembled:  # (the device policy can write x0 itself: amx_policy_act's fused assembly)
            N.check(c.lib.amx_assemble_input(c.h, ob.data_ptr(), act.data_ptr(), dt, buf.data_ptr(), Bp * c.ldk,
                                             c.ldk, B, s), "amx_assemble_input")
        self._mlp(buf, preds, Bp, s, rexp, row_exponents=assembled, k_shared=k_shared)
        return preds

    def _mlp_h3(self, buf, preds, Bp, s, rexp, k_shared=0):
        c = self.ctx
        sA, sR, L = Bp * c.ldk, (c.L + 1) * Bp, c.L
        if self.plain:
            return self._mlp_h3_plain(buf, preds, Bp, s, rexp, sA, sR, Bp * c.S, k_shared)
        for i in range(L):
            K = c.k0_pad + i * c.Hp
            N.check(c.lib.amx_gemm_bias_act_h3(c.h, c.M, Bp, c.Hp, K, buf.data_ptr(), c.ldk, sA, self.W2[i].data_ptr(),
                                               c.Hp * 2 * K, self.wexp[i].data_ptr(), c.Hp, self.b[i].data_ptr(), c.Hp,
                                               buf.data_ptr(), c.ldk, sA, K, N.AMX_ACT_RELU, rexp.data_ptr(), sR,
                                               i + 1, rexp[0, i + 1].data_ptr(), k_shared, s), "amx_gemm_bias_act_h3")
        N.check(c.lib.amx_gemm_out_unnorm_h3(c.h, c.M, Bp, c.S, c.ldk, buf.data_ptr(), c.ldk, sA,
                                             self.W2[L].data_ptr(), c.n_out_pad * 2 * c.ldk, self.wexp[L].data_ptr(),
                                             c.n_out_pad, self.b[L].data_ptr(), c.n_out_pad, preds.data_ptr(), c.S,
                                             Bp * c.S, rexp.data_ptr(), sR, L + 1, k_shared, s),
                "amx_gemm_out_unnorm_h3")

    def _mlp(self, buf, preds, Bp, s, rexp, row_exponents=True, k_shared=0):
        c = self.ctx
        sA = Bp * c.ldk
        if self.W2 is not None and row_exponents:  # x0 row exponents (slot 0) + reset of the hidden slots
            N.check(c.lib.amx_row_exponents(c.h, c.M, Bp, c.k0_pad, buf.data_ptr(), c.ldk, sA, rexp.data_ptr(),
                                            (c.L + 1) * Bp, c.L + 1, s), "amx_row_exponents")
        ev = self.gemm_events
        if ev is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if self.W2 is not None:
            self._mlp_h3(buf, preds, Bp, s, rexp, k_shared)
            if ev is not None:
                e1.record()
                ev.append((e0, e1, Bp))
            return
        win = self.layer_windows()  # (first column, K) per layer: the operand by pointer, K and ldk
        for i in range(c.L):
            (c0, K), col = win[i], c.k0_pad + i * c.Hp
            a0 = buf.data_ptr() + 4 * c0
            if self.W3 is not None:
                N.check(c.lib.amx_gemm_bias_act_x6(c.h, c.M, Bp, c.Hp, K, a0, c.ldk, sA,
                                                   self.W3[i].data_ptr(), c.Hp * 3 * K, self.b[i].data_ptr(), c.Hp,
                                                   buf.data_ptr(), c.ldk, sA, col, N.AMX_ACT_RELU, s),
                        "amx_gemm_bias_act_x6")
            else:
                N.check(c.lib.amx_gemm_bias_act(c.h, c.M, Bp, c.Hp, K, a0, c.ldk, sA, self.W[i].data_ptr(),
                                                K, c.Hp * K, self.b[i].data_ptr(), c.Hp, buf.data_ptr(), c.ldk, sA,
                                                col, N.AMX_ACT_RELU, s), "amx_gemm_bias_act")
        c0, K = win[c.L]
        a0 = buf.data_ptr() + 4 * c0
        if self.W3 is not None:
            N.check(c.lib.amx_gemm_out_unnorm_x6(c.h, c.M, Bp, c.S, K, a0, c.ldk, sA,
                                                 self.W3[c.L].data_ptr(), c.n_out_pad * 3 * K,
                                                 self.b[c.L].data_ptr(), c.n_out_pad, preds.data_ptr(), c.S,
                                                 Bp * c.S, s), "amx_gemm_out_unnorm_x6")
        else:
            N.check(c.lib.amx_gemm_out_unnorm(c.h, c.M, Bp, c.S, K, a0, c.ldk, sA,
                                              self.W[c.L].data_ptr(), K, c.n_out_pad * K,
                                              self.b[c.L].data_ptr(), c.n_out_pad, preds.data_ptr(), c.S, Bp * c.S, s),
                    "amx_gemm_out_unnorm")
        if ev is not None:
            e1.record()
            ev.append((e0, e1, Bp))

    def mlp_flops_per_sample(self) -> int:
        """Algorithmic FLOPs of one sample through all members (unpadded shapes)."""
        c, h = self.ctx, self.hidden
        if self.plain:
            macs = h * (c.S + c.A) + (c.L - 1) * h * h + c.S * h
        else:
            macs = sum(h * (c.S + c.A + i * h) for i in range(c.L)) + c.S * (c.S + c.A + c.L * h)
        return 2 * macs * c.M

    def disagreement(self, preds: torch.Tensor, B: int, out: torch.Tensor | None = None) -> torch.Tensor:
        c = self.ctx
        out = torch.empty(B, dtype=torch.float32, device=c.device) if out is None else out
        N.check(c.lib.amx_disagreement(c.h, preds.data_ptr(), c.S, preds.shape[1] * c.S, out.data_ptr(), B, c.stream),
                "amx_disagreement")
        return out

    # ---- reference-compatible surface (milo/milo/dynamics.py) ------------------------------
    def get_action_discrepancy(self, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        """DynamicsEnsemble.get_action_discrepancy (dynamics.py:154-165): float32 inputs,
        returns the per-row max pairwise L2 disagreement [B] (on the device)."""
        state = state.to(self.ctx.device, torch.float32).contiguous()
        action = action.to(self.ctx.device, torch.float32).contiguous()
        if state.dim() == 1:
            state, action = state.unsqueeze(0), action.unsqueeze(0)
        B = state.shape[0]
        preds = self.forward_preds(state, action, B)
        return self.disagreement(preds, B)

    def compute_threshold(self, states: torch.Tensor, actions: torch.Tensor, batch: int = 65536) -> float:
        """compute_threshold (dynamics.py:145-152): max disagreement over the offline set."""
        best = None
        for i in range(0, states.shape[0], batch):
            d = self.get_action_discrepancy(states[i:i + batch], actions[i:i + batch]).max()
            best = d if best is None else torch.maximum(best, d)
        self.threshold = float(best.item())
        return self.threshold

    def model_forward(self, k: int, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        """models[k].forward(state, action, unnormalize_out=True) (dynamics.py:216-233)."""
        state = state.to(self.ctx.device, torch.float32).contiguous()
        action = action.to(self.ctx.device, torch.float32).contiguous()
        B = state.shape[0]
        return self.forward_preds(state, action, B)[k, :B].clone()


    # ---- training (DynamicsModel.train_step / validate_step, dynamics.py:236-261) ------------
    _fit = None  # training state, allocated by fit_begin

    def fit_begin(self, train_data, optim: str, lr: float, p1: float, batch_size: int, val_data=None,
                  opt_state=None, num_models: int | None = None, hidden_sizes=None) -> None:
        """Allocate the training state (gradients, optimizer state in the padded layout, the step
        workspace for batches of `batch_size`, the datasets on the device) and upload `opt_state`
        (per member {'step': int, 's1': [(W, b), ...], 's2': [...]} in nn.Linear layout, or None
        for a fresh optimizer).  `train_data` / `val_data` = (states, actions, next_states).
        optim 'adam' (p1 = eps) or 'sgd' (p1 = momentum, nesterov).  Everything is validated
        before anything is allocated or launched."""
        c = self.ctx
        if num_models is not None and num_models != c.M:
            raise ValueError(f"training {num_models} members on a context of {c.M}")
        if hidden_sizes is not None and (len(set(hidden_sizes)) != 1 or len(hidden_sizes) != c.L
                                         or hidden_sizes[0] != self.hidden):
            raise NotImplementedError(f"the device ensemble trains equal hidden widths ({c.L} x {self.hidden}), "
                                      f"got {list(hidden_sizes)}")
        if optim not in ("adam", "sgd"):
            raise NotImplementedError(f"optimizer {optim!r} (supported: 'adam', 'sgd')")
        if not lr > 0 or (optim == "adam" and not p1 > 0) or (optim == "sgd" and not p1 >= 0):
            raise ValueError(f"lr={lr}, {'eps' if optim == 'adam' else 'momentum'}={p1}")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size={batch_size}")
        data = {}
        for name, d in (("train", train_data), ("val", val_data)):
            if d is None:
                continue
            s, a, s2 = [torch.as_tensor(x) for x in d]
            n = s.shape[0]
            if n < 1 or tuple(s.shape) != (n, c.S) or tuple(a.shape) != (n, c.A) or tuple(s2.shape) != (n, c.S):
                raise ValueError(f"{name} data: shapes {tuple(s.shape)}, {tuple(a.shape)}, {tuple(s2.shape)} do not "
                                 f"match S={c.S}, A={c.A}")
            data[name] = (s, a, s2)
        host = None
        if opt_state is not None:
            if len(opt_state) != c.M:
                raise ValueError(f"optimizer state of {len(opt_state)} members, expected {c.M}")
            host = [pack_state(self.layout, optim, [(0, a, b) for a, b in zip(flat_pairs(st.get("s1"), c.L),
                                                                               flat_pairs(st.get("s2"), c.L))])
                    for st in opt_state]
        P = int(c.lib.amx_efit_param_count(c.h))
        Bt = round_up(int(batch_size), 128)
        floats = int(c.lib.amx_efit_work_floats(c.h, Bt))
        if P <= 0 or floats <= 0:
            raise N.AmxNativeError("amx_efit sizes: " + c.lib.amx_last_error().decode())
        assert P == self.layout.size
        dev = c.device
        f = dict(optim=optim, lr=float(lr), p1=float(p1), batch_size=int(batch_size), Bt=Bt, P=P)
        f["data"] = {k: tuple(x.detach().to(dev, torch.float32).contiguous() for x in v) for k, v in data.items()}
        f["grad"] = torch.zeros(c.M, P, dtype=torch.float32, device=dev)
        f["s1"] = torch.zeros(c.M, P, dtype=torch.float32, device=dev)
        f["s2"] = torch.zeros(c.M, P, dtype=torch.float32, device=dev) if optim == "adam" else None
        f["step"] = torch.zeros(c.M, dtype=torch.int64, device=dev)
        f["work"] = torch.zeros(floats, dtype=torch.float32, device=dev)
        f["Wp"] = (N.C.c_void_p * (c.L + 1))(*[w.data_ptr() for w in self.W])
        f["bp"] = (N.C.c_void_p * (c.L + 1))(*[b.data_ptr() for b in self.b])
        if host is not None:
            f["step"].copy_(torch.tensor([int(st["step"]) for st in opt_state], dtype=torch.int64))
            f["s1"].copy_(torch.stack([s1 for s1, _ in host]))
            if f["s2"] is not None:
                f["s2"].copy_(torch.stack([s2 for _, s2 in host]))
        self._fit = f

    def fit_epoch(self, idx, sizes, train: bool = True, grad_clip: float = 0.0, split: str = "train") -> np.ndarray:
        """One pass of every member over its own batches, in lock step: `idx` int32
        [M][steps][batch_size] (member g's step s takes rows idx[g, s, :sizes[s]] of the
        `split` data), train steps or validation steps (gather, forward and loss only).
        Returns the step losses [M][steps] (float32; one synchronisation, at the end)."""
        f, c = self._fit, self.ctx
        if f is None:
            raise RuntimeError("fit_epoch before fit_begin")
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        steps = len(sizes)
        if idx.shape != (c.M, steps, f["batch_size"]) or any(not 1 <= n <= f["batch_size"] for n in sizes):
            raise ValueError(f"idx {idx.shape} / sizes do not match [{c.M}][{steps}][{f['batch_size']}]")
        if not grad_clip >= 0:
            raise ValueError(f"grad_clip={grad_clip}")
        s_, a_, s2_ = f["data"][split]
        d_idx = torch.from_numpy(idx).to(c.device)
        loss = torch.zeros(c.M, steps, dtype=torch.float32, device=c.device)
        bs, s2p = f["batch_size"], (f["s2"].data_ptr() if f["s2"] is not None else None)
        opt = N.AMX_EFIT_ADAM if f["optim"] == "adam" else N.AMX_EFIT_SGD
        stream = c.stream
        for s in range(steps):
            N.check(c.lib.amx_efit_step(c.h, int(train), int(sizes[s]), f["Bt"], d_idx.data_ptr() + 4 * s * bs,
                                        steps * bs, s_.shape[0], s_.data_ptr(), a_.data_ptr(), s2_.data_ptr(),
                                        f["Wp"], f["bp"], f["grad"].data_ptr(), f["s1"].data_ptr(), s2p,
                                        f["step"].data_ptr(), opt, f["lr"], f["p1"], float(grad_clip),
                                        loss.data_ptr() + 4 * s, steps, f["work"].data_ptr(), stream),
                    "amx_efit_step")
        return loss.cpu().numpy()

    def fit_state(self):
        """The device training state in nn.Linear layout: (weights, opt_state) with weights[m] =
        [(W, b), ...] and opt_state[m] = {'step', 's1', 's2'} as fit_begin takes them."""
        f, c = self._fit, self.ctx
        padded = [t.cpu().reshape(c.M, -1) for Wb in zip(self.W, self.b) for t in Wb]
        host = {"W": torch.cat(padded, 1), "s1": f["s1"].cpu(), "s2": None if f["s2"] is None else f["s2"].cpu()}
        steps = f["step"].cpu().tolist()

        def live(key, m):  # [(W, b), ...] of member m in nn.Linear layout
            if host[key] is None:
                return None
            t = self.layout.unpack(host[key][m])
            return list(zip(t[0::2], t[1::2]))

        weights = [live("W", m) for m in range(c.M)]
        return weights, [{"step": int(steps[m]), "s1": live("s1", m), "s2": live("s2", m)} for m in range(c.M)]

    def fit_refresh(self) -> None:
        """Re-split the inference limb images from the trained master weights, in place: engines
        and captured graphs that hold their pointers see the trained model."""
        for i in range(self.ctx.L + 1):
            if self.W3 is not None:
                split_bf16x3(self.ctx, self.W[i], out=self.W3[i])
            if self.W2 is not None:
                split_f16x2(self.ctx, self.W[i], out=(self.W2[i], self.wexp[i]))

    def fit_end(self) -> None:
        """Free the training state."""
        self._fit = None


class RffMap:
    """phi(x) = cos(x W^T + b) * sqrt(2/F) on MFMA (linear_cost.py:64-71) with fp64 column sums."""

    step_invariant = True  # one launch whose per-row work does not depend on the row count

    def __init__(self, ctx: AmxContext, W: torch.Tensor, b: torch.Tensor, gemm: str = "f16x3"):
        """gemm: "f16x3" (amx_rff_features_h3 on the scaled 2-limb image of W), "bf16x6"
        (amx_rff_features_x6 on the 3-limb image) or "f32"."""
        if gemm not in DeviceEnsemble.GEMM_PRECISIONS:
            raise ValueError(f"gemm must be one of {DeviceEnsemble.GEMM_PRECISIONS}, got {gemm!r}")
        self.gemm = gemm
        self.ctx = ctx
        F, D = W.shape
        self.F, self.D = F, D
        self.Fp = round_up(F, 128)
        if self.Fp != F:
            raise ValueError("feature_dim must be a multiple of 128 for the MFMA RFF path")
        self.Kp = round_up(D, 32)
        Wp = torch.zeros(F, self.Kp, dtype=torch.float32)
        Wp[:, :D] = W.float().cpu()
        self.W = Wp.to(ctx.device).contiguous()
        self.b = b.float().to(ctx.device).contiguous()
        self.W3 = split_bf16x3(ctx, self.W.unsqueeze(0))[0] if gemm == "bf16x6" else None
        self.W2 = self.wexp = None
        if gemm == "f16x3":
            W2, wexp = split_f16x2(ctx, self.W.unsqueeze(0))
            self.W2, self.wexp = W2[0], wexp[0]
        # np.sqrt(2/F) is a float64 scalar; torch multiplies the fp32 tensor by it rounded to fp32
        self.scale = float(np.float32(np.sqrt(2 / F)))

    def features(self, x: torch.Tensor, rows: int, n_valid: int, phi: torch.Tensor, partials: torch.Tensor,
                 row_mask: torch.Tensor | None = None, ldx: int | None = None,
                 row_exp: torch.Tensor | None = None) -> None:
        """phi rows + fp64 column partials [rows / 32][F] (one per 32-row group, AMX_RFF_PART_ROWS)
        of x's `rows` rows.  f16x3: `row_exp` [rows] int32 = the rows' exponents (amx_step_rexp
        writes them for the rollout's [s, s'] rows); None computes them here (amx_row_exponents)."""
        c = self.ctx
        if partials.dtype != torch.float64 or partials.numel() < rows // N.RFF_PART_ROWS * self.F:
            raise ValueError(f"partials must be fp64 with room for [{rows // N.RFF_PART_ROWS}][{self.F}] "
                             f"(one row per {N.RFF_PART_ROWS} feature rows), got {tuple(partials.shape)} "
                             f"{partials.dtype}")
        ldx = self.Kp if ldx is None else ldx
        if self.W2 is not None:
            if row_exp is None:
                row_exp = torch.empty(rows, dtype=torch.int32, device=c.device)
                N.check(c.lib.amx_row_exponents(c.h, 1, rows, self.Kp, x.data_ptr(), ldx, 0, row_exp.data_ptr(), rows,
                                                1, c.stream), "amx_row_exponents")
            N.check(c.lib.amx_rff_features_h3(c.h, rows, n_valid, self.F, self.Kp, x.data_ptr(), ldx,
                                              self.W2.data_ptr(), self.wexp.data_ptr(), row_exp.data_ptr(),
                                              self.b.data_ptr(), self.scale, phi.data_ptr(), phi.shape[-1],
                                              partials.data_ptr(), None if row_mask is None else row_mask.data_ptr(),
                                              c.stream), "amx_rff_features_h3")
            return
        if self.W3 is not None:
            N.check(c.lib.amx_rff_features_x6(c.h, rows, n_valid, self.F, self.Kp, x.data_ptr(), ldx,
                                              self.W3.data_ptr(), self.b.data_ptr(), self.scale, phi.data_ptr(),
                                              phi.shape[-1], partials.data_ptr(),
                                              None if row_mask is None else row_mask.data_ptr(), c.stream),
                    "amx_rff_features_x6")
            return
        N.check(c.lib.amx_rff_features(c.h, rows, n_valid, self.F, self.Kp, x.data_ptr(), ldx, self.W.data_ptr(),
                                       self.Kp, self.b.data_ptr(), self.scale, phi.data_ptr(), phi.shape[-1],
                                       partials.data_ptr(), None if row_mask is None else row_mask.data_ptr(),
                                       c.stream), "amx_rff_features")

    def embed(self, x: torch.Tensor):
        """(phi [n, F], column sums [F] fp64) of arbitrary rows x [n, D] (fp32, any device)."""
        c = self.ctx
        n = x.shape[0]
        rows = round_up(max(n, 1), 128)
        # the 160 x 256 one-round tiles (amx_rff_features_h3) need rows = k * 160 * CUs / (F / 256):
        # worth ~1 % of padding rows (40 530 -> 40 960: 121 -> 76 us on 128 x 128 tiles)
        r160 = 160 * c.n_cus // max(self.F // 256, 1) if self.F % 256 == 0 else 0
        if self.W2 is not None and r160 and n >= r160 and round_up(n, r160) <= 1.05 * n:
            rows = round_up(n, r160)
        xp = torch.zeros(rows, self.Kp, dtype=torch.float32, device=c.device)
        xp[:n, :self.D] = x.to(c.device, torch.float32)
        phi = torch.empty(rows, self.F, dtype=torch.float32, device=c.device)
        part = torch.empty(rows // N.RFF_PART_ROWS, self.F, dtype=torch.float64, device=c.device)
        self.features(xp, rows, n, phi, part)
        tot = torch.empty(self.F, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_sum_partials(c.h, part.data_ptr(), rows // N.RFF_PART_ROWS, self.F, tot.data_ptr(), c.stream),
                "amx_sum_partials")
        return phi[:n], tot


class MlpMap:
    """phi(x) = cos(tanh(net(x))) * sqrt(2/F), net = Linear, [ReLU, Linear]... (MLPCost.get_rep,
    linear_cost.py:199-212, 232-237), with RffMap's interface: the hidden layers are
    amx_gemm_bias_act_h3 launches chained through their row exponents, the last Linear runs in
    amx_mlp_features_h3 (phi rows + fp64 column partials).  f16x3 only."""

    # the hidden layers' tiles depend on the row count, so scoring one step's rows at a time
    # rounds differently from one pass over the rollout (RolloutEngine.rollout's score_overlap)
    step_invariant = False

    def __init__(self, ctx: AmxContext, layers):
        """`layers` = [(W, b), ...] in nn.Linear layout, the last one the feature layer.  Hidden
        widths are zero-padded to multiples of 128 (zero weight rows and zero bias: ReLU keeps the
        pad at 0, and the next layer's pad columns are zero)."""
        self.ctx = ctx
        F, D = int(layers[-1][0].shape[0]), int(layers[0][0].shape[1])
        if round_up(F, 128) != F:
            raise ValueError("feature_dim must be a multiple of 128 for the MFMA feature path")
        self.F, self.D = F, D
        self.Kp = round_up(D, 32)
        self.gemm = "f16x3"
        self.layers = []   # (W2, wexp, bias, out_p, k_pad) per Linear
        k, k_pad = D, self.Kp
        for W, b in layers:
            out, kin = int(W.shape[0]), int(W.shape[1])
            if kin != k or tuple(b.shape) != (out,):
                raise ValueError(f"layer shapes {tuple(W.shape)} / {tuple(b.shape)} do not chain (expected {k} inputs)")
            out_p = round_up(out, 128)
            Wp = torch.zeros(out_p, k_pad, dtype=torch.float32)
            Wp[:out, :k] = W.detach().float().cpu()
            bp = torch.zeros(out_p, dtype=torch.float32)
            bp[:out] = b.detach().float().cpu()
            W2, wexp = split_f16x2(ctx, Wp.to(ctx.device).unsqueeze(0))
            self.layers.append((W2[0], wexp[0], bp.to(ctx.device), out_p, k_pad))
            k, k_pad = out, out_p
        self.n_hidden = len(self.layers) - 1
        self.h_max = max([L[3] for L in self.layers[:-1]], default=0)
        self.W2, self.wexp = self.layers[0][0], self.layers[0][1]
        # np.sqrt(2/F) is a float64 scalar; torch multiplies the fp32 tensor by it rounded to fp32
        self.scale = float(np.float32(np.sqrt(2 / F)))
        self._ws = {}

    def _workspace(self, rows: int, cache: bool = True):
        """Two ping-pong hidden buffers [rows][h_max] and the exponent slots [1 + n_hidden][rows]
        (slot 0: the input rows, slot i + 1: hidden layer i's output rows)."""
        ws = self._ws.get(rows)
        if ws is None:
            dev = self.ctx.device
            ws = ([torch.empty(rows * self.h_max, dtype=torch.float32, device=dev) for _ in range(min(self.n_hidden, 2))],
                  torch.empty(1 + self.n_hidden, rows, dtype=torch.int32, device=dev))
            if cache:
                self._ws[rows] = ws
        return ws

    def features(self, x: torch.Tensor, rows: int, n_valid: int, phi: torch.Tensor, partials: torch.Tensor,
                 row_mask: torch.Tensor | None = None, ldx: int | None = None,
                 row_exp: torch.Tensor | None = None, cache: bool = True) -> None:
        """phi rows + fp64 column partials [rows / 32][F] of x's `rows` rows (RffMap.features'
        contract).  `row_exp` [rows] int32 = the input rows' exponents (amx_step_rexp writes them
        for the rollout's [s, s'] rows); None computes them here.  The buffers are cached per row
        count: after the first call at a row count nothing is allocated and nothing synchronises
        (`cache=False`: one-off buffers, for embed's arbitrary row counts)."""
        c = self.ctx
        if partials.dtype != torch.float64 or partials.numel() < rows // N.RFF_PART_ROWS * self.F:
            raise ValueError(f"partials must be fp64 with room for [{rows // N.RFF_PART_ROWS}][{self.F}] "
                             f"(one row per {N.RFF_PART_ROWS} feature rows), got {tuple(partials.shape)} "
                             f"{partials.dtype}")
        bufs, rexp = self._workspace(rows, cache)
        h, ldh = x, (self.Kp if ldx is None else ldx)
        if row_exp is None:
            N.check(c.lib.amx_row_exponents(c.h, 1, rows, self.Kp, h.data_ptr(), ldh, 0, rexp.data_ptr(), rows, 1,
                                            c.stream), "amx_row_exponents(mlp)")
            row_exp = rexp[0]
        if self.n_hidden:
            rexp[1:].fill_(-100)   # the hidden epilogues max into their slots
        for i, (W2, wexp, b, out_p, k_pad) in enumerate(self.layers[:-1]):
            o = bufs[i & 1]
            N.check(c.lib.amx_gemm_bias_act_h3(c.h, 1, rows, out_p, k_pad, h.data_ptr(), ldh, 0, W2.data_ptr(), 0,
                                               wexp.data_ptr(), 0, b.data_ptr(), 0, o.data_ptr(), out_p, 0, 0,
                                               N.AMX_ACT_RELU, row_exp.data_ptr(), 0, 1, rexp[i + 1].data_ptr(), 0,
                                               c.stream), "amx_gemm_bias_act_h3(mlp)")
            h, ldh, row_exp = o, out_p, rexp[i + 1]
        W2, wexp, b, _, k_pad = self.layers[-1]
        N.check(c.lib.amx_mlp_features_h3(c.h, rows, n_valid, self.F, k_pad, h.data_ptr(), ldh, W2.data_ptr(),
                                          wexp.data_ptr(), row_exp.data_ptr(), b.data_ptr(), self.scale,
                                          phi.data_ptr(), phi.shape[-1], partials.data_ptr(),
                                          None if row_mask is None else row_mask.data_ptr(), c.stream),
                "amx_mlp_features_h3")

    def embed(self, x: torch.Tensor):
        """(phi [n, F], column sums [F] fp64) of arbitrary rows x [n, D] (fp32, any device)."""
        c = self.ctx
        n = x.shape[0]
        rows = round_up(max(n, 1), 128)
        # whole rounds of the feature layer's 160 x 256 tiles where ~1 % of padding buys them
        # (RffMap.embed), when that row count also suits the hidden layers' 128-row tiles
        r160 = 160 * c.n_cus // max(self.F // 256, 1) if self.F % 256 == 0 else 0
        if r160 and r160 % 128 == 0 and n >= r160 and round_up(n, r160) <= 1.05 * n:
            rows = round_up(n, r160)
        xp = torch.zeros(rows, self.Kp, dtype=torch.float32, device=c.device)
        xp[:n, :self.D] = x.to(c.device, torch.float32)
        phi = torch.empty(rows, self.F, dtype=torch.float32, device=c.device)
        part = torch.empty(rows // N.RFF_PART_ROWS, self.F, dtype=torch.float64, device=c.device)
        self.features(xp, rows, n, phi, part, cache=False)
        tot = torch.empty(self.F, dtype=torch.float64, device=c.device)
        N.check(c.lib.amx_sum_partials(c.h, part.data_ptr(), rows // N.RFF_PART_ROWS, self.F, tot.data_ptr(), c.stream),
                "amx_sum_partials")
        return phi[:n], tot
