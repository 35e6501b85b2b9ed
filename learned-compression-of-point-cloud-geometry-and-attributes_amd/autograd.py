"""Differentiable sparse convolution (training path).

The reference trains through MinkowskiEngine's autograd functions (every ``ME.Minkowski*Convolution*``
in model/, driven by train.py:194-206).  Here one ``torch.autograd.Function`` wraps the HIP kernels:

    forward   out = bias + sum_k X[nbr[:, k]] @ W[k]                      pcc_conv_fwd
    backward  dX  = the same kernel over the transposed map with W[k]^T   pcc_kernel_map_transpose + pcc_conv_fwd
              dW[k] = sum over pairs of X[i]^T dY[j]                      pcc_conv_wgrad
              db  = column sums of dY

Maps, launches and packed weights are the inference path's (sparse.py: ``CoordMap.conv_map``, ``launch_conv``, the layer's cached
``weights``); this module adds what autograd needs.

The channelwise window convolution of the ColorSSIM loss (``ChannelwiseConvFn``) is its own node on pcc_chconv: forward
with the window as given, backward-data the same kernel on dY with the window flipped.

Activations, FiLM and residuals — fused into the convolution's epilogue on the inference path — are
ordinary torch ops here so that autograd differentiates them.
"""
import os

import torch

from . import _lib
from ._lib import check, ptr
from .sparse import ACT_LRELU, ACT_RELU, MODE_BF16, MODE_F32, _plan_takes, launch_conv, launch_mode, pack_weights

# bf16 compute for the training path (BASELINE config 5: "bf16"): convolutions whose input width is a multiple of
# 64 cast their input (forward: the features; backward-data: the output gradient) and weights to bf16 and run on
# v_mfma_f32_32x32x16_bf16 with fp32 accumulation and fp32 outputs; everything else — narrow and thin layers,
# the entropy models, the losses, the master weights — stays fp32; weight gradients of layers with both widths
# multiples of 64 take bf16 operands too (fp32 sums).  Off by default.
BF16 = os.environ.get("PCC_TRAIN_BF16", "0") == "1"


def set_bf16(enabled):
    global BF16
    BF16 = bool(enabled)


# Split-bf16 arithmetic for the fp32 training step (opt-in, PCC_TRAIN_X3=1 / set_x3): forward and backward-data
# convolutions with fp32 data run their products as six bf16 MFMA terms of an exact three-way split (csrc/conv.hip, X3):
# fp32-class values at 3/8 of the fp32 MFMA time.  Weight gradients stay on the fp32 kernel.  Ignored where BF16 applies.
X3 = os.environ.get("PCC_TRAIN_X3", "0") == "1"


def set_x3(enabled):
    global X3
    X3 = bool(enabled)


def _mode(rows, cin, cout, n_out, K, has_nbr):
    """the arithmetic of a training-path launch of this shape (fp32 unless PCC_TRAIN_BF16 / PCC_TRAIN_X3 ask otherwise)"""
    return launch_mode(BF16, X3, rows, cin, cout, n_out, K, has_nbr) if BF16 or X3 else MODE_F32


def _taken_width(n_out, cout, cin, n_in, K, has_nbr):
    """backward-data reads dY as its input: the first width >= cout that the fp32 plan takes (narrow dY is zero-padded to it)"""
    return next((c for c in range(cout, cout + 32) if _plan_takes(MODE_F32, n_out, c, cin, n_in, K, has_nbr)), cout)


class SparseConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, kernel, bias, layer, in_map, out_map, ksize, transposed, out_channels):
        feats = feats.contiguous()
        w, _, b = layer.weights(out_channels)
        nbr, order, gmask, _ = in_map.conv_map(out_map, ksize, transposed, feats.shape[1])
        mode = _mode(feats.shape[0], w.shape[1], w.shape[2], out_map.n, w.shape[0], nbr is not None)
        if mode == MODE_BF16:
            feats = feats.to(torch.bfloat16)          # the one cast of this tensor: forward now, weight gradient later
        out = torch.empty((out_map.n, w.shape[2]), dtype=torch.float32, device=feats.device)
        launch_conv(mode, feats, w, layer.packed(mode, out_channels), b, nbr, order, gmask, out)
        ctx.save_for_backward(feats, w)
        ctx.meta = (in_map, out_map, ksize, transposed, out_channels, tuple(kernel.shape), bias is not None)
        return out

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        feats, w = ctx.saved_tensors
        in_map, out_map, ksize, transposed, out_channels, kshape, has_bias = ctx.meta
        dy = dy.contiguous()
        K, cin, cout = w.shape
        n_in, n_out = feats.shape[0], dy.shape[0]
        dev = dy.device
        d_feats = d_kernel = d_bias = None
        bf = feats.dtype == torch.bfloat16                 # forward ran in bf16: the saved input is the bf16 copy
        want_db = has_bias and ctx.needs_input_grad[2]
        # dY is read once for its bf16 copy (weight gradient, backward-data) and its column sums (bias gradient)
        dy_bf = db = None
        if (want_db or (bf and ctx.needs_input_grad[1])) and cout % 4 == 0 and cout <= 1024:
            if bf and ctx.needs_input_grad[1]:
                dy_bf = torch.empty((n_out, cout), dtype=torch.bfloat16, device=dev)
            if want_db:
                db = torch.empty(cout, dtype=torch.float32, device=dev)
            ne_cs = L.pcc_cast_colsum_scratch_elems(cout)
            cs_scratch = torch.empty(ne_cs if want_db else 0, dtype=torch.float32, device=dev)
            check(L.pcc_cast_colsum(ptr(dy), n_out, cout, ptr(dy_bf), ptr(db), ptr(cs_scratch) if want_db else None, ne_cs,
                                    _lib.stream()))

        if ctx.needs_input_grad[1]:
            # Thin shapes (q-map branches, input layer, narrow heads) are zero-padded to 32 channels and take the MFMA
            # kernel too: the scalar kernel walks its rows serially and needs 60 ms for 2 -> 128 on 3.4 M rows where
            # the padded MFMA launch takes 7 (16x the multiplications, all of them in the matrix pipe).
            unit = 64 if bf else 32
            cin_p, cout_p = (cin + unit - 1) // unit * unit, (cout + unit - 1) // unit * unit
            x_w = feats
            g_w = (dy_bf if dy_bf is not None else dy.to(torch.bfloat16)) if bf else dy
            if cin_p != cin:
                x_w = torch.cat([x_w, torch.zeros((n_in, cin_p - cin), dtype=x_w.dtype, device=dev)], dim=1)
            if cout_p != cout:
                g_w = torch.cat([g_w, torch.zeros((n_out, cout_p - cout), dtype=g_w.dtype, device=dev)], dim=1)
            if ksize == 1:
                nbr = torch.arange(n_out, dtype=torch.int32, device=dev).unsqueeze(1).contiguous()
                order = gmask = None
            else:
                nbr, order, gmask, _ = in_map.position_ordered_table(out_map, ksize, transposed)      # the wgrad kernels index by position
            dw = torch.empty((K, cin_p, cout_p), dtype=torch.float32, device=dev)
            ne = L.pcc_conv_wgrad_scratch_elems(K, cin_p, cout_p)
            scratch = torch.empty(ne, dtype=torch.float32, device=dev)
            if bf:
                check(L.pcc_conv_wgrad_bf16(ptr(x_w), n_in, cin_p, ptr(g_w), n_out, cout_p, ptr(nbr), ptr(order), ptr(gmask), K, ptr(dw),
                                            ptr(scratch), ne, _lib.stream()))
            else:
                check(L.pcc_conv_wgrad(ptr(x_w), n_in, cin_p, ptr(g_w), n_out, cout_p, ptr(nbr), ptr(order), ptr(gmask), K, ptr(dw),
                                       ptr(scratch), ne, _lib.stream()))
            if cin_p != cin or cout_p != cout:
                dw = dw[:, :cin, :cout].contiguous()
            if out_channels is not None:
                full = torch.zeros((K, cin, kshape[-1]), dtype=torch.float32, device=dev)
                full[:, :, :out_channels] = dw
                dw = full
            d_kernel = dw.reshape(kshape)

        if want_db:
            if db is None:
                db = dy.sum(dim=0)
            if out_channels is not None:
                full = torch.zeros(kshape[-1], dtype=torch.float32, device=dev)
                full[:out_channels] = db
                db = full
            d_bias = db.reshape(1, -1)

        if ctx.needs_input_grad[0]:
            wt = w.transpose(1, 2)                                  # [K, cout, cin]
            g = dy
            width = _taken_width(n_out, cout, cin, n_in, K, ksize > 1)
            if width != cout:
                g = torch.cat([dy, torch.zeros((n_out, width - cout), dtype=torch.float32, device=dev)], dim=1).contiguous()
                wt = torch.cat([wt, torch.zeros((K, width - cout, cin), dtype=torch.float32, device=dev)], dim=1)
            wt = wt.contiguous()
            mode = _mode(n_out, width, cin, n_in, K, ksize > 1)
            if mode == MODE_BF16 and bf and ctx.needs_input_grad[1]:
                g = g_w                                             # the bf16 copy the weight gradient made
            nbr_t, order_t, gmask_t, _ = in_map.conv_map(out_map, ksize, transposed, width, adjoint=True)
            d_feats = torch.empty((n_in, cin), dtype=torch.float32, device=dev)
            launch_conv(mode, g, wt, pack_weights(wt, mode), None, nbr_t, order_t, gmask_t, d_feats)
        return d_feats, d_kernel, d_bias, None, None, None, None, None, None


class EpilogueFn(torch.autograd.Function):
    """out = act(c * beta + gamma) + residual as ONE kernel forward and ONE backward (csrc/epilogue.hip) — the terms the
    inference path fuses into the convolution's epilogue; same operation order, hence the same values and gradients, as
    the chain of torch ops this replaces"""

    @staticmethod
    def forward(ctx, c, film, residual, act):
        c = c.contiguous()
        film = None if film is None else film.contiguous()
        residual = None if residual is None else residual.contiguous()
        n, ch = c.shape
        out = torch.empty_like(c)
        check(_lib.lib().pcc_epilogue_fwd(ptr(c), ptr(film), ptr(residual), n, ch, act, ptr(out), _lib.stream()))
        ctx.save_for_backward(c, film)
        ctx.act = act
        ctx.has_res = residual is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        c, film = ctx.saved_tensors
        dout = dout.contiguous()
        n, ch = c.shape
        dc = torch.empty_like(c)
        dfilm = None if film is None else torch.empty_like(film)
        check(_lib.lib().pcc_epilogue_bwd(ptr(dout), ptr(c), ptr(film), n, ch, ctx.act, ptr(dc), ptr(dfilm), _lib.stream()))
        return dc, dfilm, (dout if ctx.has_res else None), None


def epilogue_train(c, film, residual, act):
    """differentiable epilogue; falls back to torch ops for shapes the kernel does not take (channels % 4 != 0)"""
    ch = c.shape[1]
    if ch % 4 == 0 and (film is None or film.shape[1] == 2 * ch):
        return EpilogueFn.apply(c, film, residual, act)
    if film is not None:
        c = c * film[:, :ch] + film[:, ch:]
    if act == ACT_RELU:
        c = torch.relu(c)
    elif act == ACT_LRELU:
        c = torch.nn.functional.leaky_relu(c, 0.01)
    return c if residual is None else c + residual


def conv_train(x_feats, in_map, out_map, layer, ksize, transposed, out_channels=None):
    """differentiable out = bias + conv(x) on the HIP kernels"""
    return SparseConvFn.apply(x_feats, layer.kernel, layer.bias, layer, in_map, out_map, ksize, transposed, out_channels)


def chconv_launch(feats, cmap, window, ksize, flip):
    """y = pcc_chconv(feats) on the set ``cmap`` with ``window`` [ksize^3, 1 or C]; flip = 1 is the adjoint"""
    n, c = feats.shape
    keys, vals, cap = cmap.table()
    out = torch.empty((n, c), dtype=torch.float32, device=feats.device)
    check(_lib.lib().pcc_chconv(ptr(feats), n, c, ptr(cmap.coords), ptr(keys), ptr(vals), cap, cmap.stride, ksize, ptr(window),
                                window.shape[1], flip, ptr(out), _lib.stream()))
    return out


class ChannelwiseConvFn(torch.autograd.Function):
    """y[i, ch] = sum_k window[k, ch] * x[nbr(i, k), ch] on one coordinate set (csrc/chconv.hip).  Input and output set are
    the same, so the backward with respect to x is the same kernel on dY with the window index reversed (flip = 1).  The
    window gets no gradient."""

    @staticmethod
    def forward(ctx, feats, window, cmap, ksize):
        ctx.save_for_backward(window)
        ctx.cmap, ctx.ksize = cmap, ksize
        return chconv_launch(feats.contiguous(), cmap, window, ksize, 0)

    @staticmethod
    def backward(ctx, dy):
        (window,) = ctx.saved_tensors
        return chconv_launch(dy.contiguous(), ctx.cmap, window, ctx.ksize, 1), None, None, None
