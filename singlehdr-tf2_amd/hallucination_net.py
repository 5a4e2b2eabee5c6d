"""Hallucination-Net on MI355X -- drop-in for the reference module of the same name.

hallucination_net.py:109-190 of the reference: VGG16-shaped encoder, bilinear-up
decoder with BatchNorm, 1x1 skip fusers.  Input NHWC float32 RGB in [0,1]
(H, W multiples of 32), output >= 0 in "BGR" order.  All arithmetic runs in the
libshdr HIP kernels; inference BatchNorm, bias, relu, the sk/255 scaling and the
channel concat are fused into the convolution.
"""
import torch

try:
    from . import _ops as K
    from ._layers import Layer, Conv2D, BatchNormalization, is_training, taping
except ImportError:
    import _ops as K
    from _layers import Layer, Conv2D, BatchNormalization, is_training, taping


class down1(Layer):
    """2 x (conv3x3 + relu) -> (maxpool2, pre-pool skip) (hallucination_net.py:43-56)."""

    def __init__(self, inChannels, outChannels, device=None):
        super().__init__()
        self.conv1 = Conv2D(inChannels, outChannels, (3, 3), device=device)
        self.conv2 = Conv2D(outChannels, outChannels, (3, 3), device=device)

    def call(self, x, proj=None):
        """proj [3, outChannels]: return (pooled, sum_c proj[j, c] skip[..., c]) -- the only use the inference tail of the network has
        for d1's skip tensor -- or None when the projection cannot be formed in the conv's epilogue"""
        if x.shape[-1] != self.conv1.kernel.shape[2]:   # zero-padded input (3 -> 4 channels)
            x = self.conv1.call_padded(x, cin_pad=x.shape[-1], act1=K.ACT_RELU)
        else:
            x = self.conv1(x, act1=K.ACT_RELU)
        if proj is not None:
            r = K.conv2d_maxpool2(x, self.conv2.kernel, self.conv2.bias, act1=K.ACT_RELU, proj=proj)
            if r is not None:
                return r[1], r[0], True
            skip_layer, pooled = K.conv2d_maxpool2(x, self.conv2.kernel, self.conv2.bias, act1=K.ACT_RELU)
            return pooled, skip_layer, False
        skip_layer, pooled = K.conv2d_maxpool2(x, self.conv2.kernel, self.conv2.bias, act1=K.ACT_RELU)
        return pooled, skip_layer


class down2(Layer):
    """3 x (conv3x3 + relu) -> (maxpool2, pre-pool skip) (hallucination_net.py:58-75)."""

    def __init__(self, inChannels, outChannels, device=None):
        super().__init__()
        self.conv1 = Conv2D(inChannels, outChannels, (3, 3), device=device)
        self.conv2 = Conv2D(outChannels, outChannels, (3, 3), device=device)
        self.conv3 = Conv2D(outChannels, outChannels, (3, 3), device=device)

    def call(self, x):
        x = self.conv1(x, act1=K.ACT_RELU)
        x = self.conv2(x, act1=K.ACT_RELU)
        skip_layer, pooled = K.conv2d_maxpool2(x, self.conv3.kernel, self.conv3.bias, act1=K.ACT_RELU)
        return pooled, skip_layer


class up(Layer):
    """bilinear 2x -> conv3x3 -> relu -> BN -> relu (hallucination_net.py:77-91).
    The reference constructs `conv2` but never calls it, so it owns no weights."""

    def __init__(self, inChannels, outChannels, device=None):
        super().__init__()
        self.conv1 = Conv2D(inChannels, outChannels, (3, 3), device=device)
        self.norm1 = BatchNormalization(outChannels, device=device)

    def call(self, x, training="training"):
        if is_training(training):       # relu(conv) -> batch-statistics BN -> relu, separate taped ops
            return self.norm1.train_apply(self.conv1(K.resize2x(x), act1=K.ACT_RELU), relu=True)
        if taping(x, self.conv1.kernel, self.norm1.gamma):     # inference mode on a tape: frozen statistics, separate tape entries
            return self.norm1.frozen_apply(self.conv1(K.resize2x(x), act1=K.ACT_RELU), relu=True)
        scale, shift = self.norm1.folded()
        # inference: resize, conv, relu, folded BN, relu in ONE kernel -- the up-sampled tensor never reaches HBM
        if x.dtype != torch.float32 or not K.WINOGRAD:
            return self.conv1.call_up2(x, act1=K.ACT_RELU, scale=scale, shift=shift, act2=K.ACT_RELU)
        # fp32: the channel mix at low resolution where the library takes the layer (csrc/up2_lowres.hip), else the call above
        return self.conv1.call_up2(x, act1=K.ACT_RELU, scale=scale, shift=shift, act2=K.ACT_RELU, lowres=True)

    def call_projected(self, x, proj):
        """tape-free inference: sum_c proj[j, c] up(x)[..., c] from the same kernel's epilogue -- the block's own output is not written --
        or None when the planned kernel cannot form it.  lowres: the one-launch low-res form where the library takes the layer (u1: 64 couts,
        csrc/up2_fused.hip), else today's bilinear-prologue kernel"""
        scale, shift = self.norm1.folded()
        return self.conv1.call_up2(x, act1=K.ACT_RELU, scale=scale, shift=shift, act2=K.ACT_RELU, proj=proj, lowres=True)


class skipLayer(Layer):
    """conv1x1(concat[x, sk/255]) (hallucination_net.py:93-107)."""

    def __init__(self, xChannels, skChannels, outChannels, device=None):
        super().__init__()
        self.conv1 = Conv2D(xChannels + skChannels, outChannels, (1, 1), device=device)

    def call(self, x, sk, **kw):
        # the 1/255 of the skip source is folded into the filter rows by the library's filter preparation (cached per parameter version)
        return self.conv1(x, x2=sk, x2_scale=1.0 / 255, **kw)


class model(Layer):
    def __init__(self, VGG_MEAN=(103.939, 116.779, 123.68), padding="SAME", device=None):
        super().__init__()
        self.VGG_MEAN = list(VGG_MEAN)
        self.d1 = down1(3, 64, device=device)
        self.d2 = down1(64, 128, device=device)
        self.d3 = down2(128, 256, device=device)
        self.d4 = down2(256, 512, device=device)
        self.d5 = down2(512, 512, device=device)
        self.conv1 = Conv2D(512, 512, (3, 3), device=device)
        self.norm1 = BatchNormalization(512, device=device)
        self.u5 = up(512, 512, device=device)
        self.s5 = skipLayer(512, 512, 512, device=device)
        self.u4 = up(512, 512, device=device)
        self.s4 = skipLayer(512, 512, 512, device=device)
        self.u3 = up(512, 256, device=device)
        self.s3 = skipLayer(256, 256, 256, device=device)
        self.u2 = up(256, 128, device=device)
        self.s2 = skipLayer(128, 128, 128, device=device)
        self.u1 = up(128, 64, device=device)
        self.s1 = skipLayer(64, 64, 64, device=device)
        self.conv2 = Conv2D(64, 3, (1, 1), device=device)
        self.norm2 = BatchNormalization(3, device=device)
        self.s0 = skipLayer(3, 3, 3, device=device)

    def call(self, input_layer, training="training"):
        train = is_training(training)
        if list(self.VGG_MEAN) != [103.939, 116.779, 123.68]:
            raise NotImplementedError("custom VGG_MEAN is not supported by the HIP preprocess kernel")
        input_layer, il = K.fork(input_layer)        # the 3-channel BGR image of the last skip layer and the padded encoder input
        bgr = K.vgg_preprocess(input_layer)          # x*255, RGB->BGR, - mean  (:149-153)
        tail, d1_projected = None, False
        # native fp16 for fine-tuning (BASELINE configs[4]) and for tape-free inference (the folded BatchNorm, the `up` blocks and the
        # composed tail run as fused fp16 epilogues: shdr_conv2d_fwd_fused_f16); inference on a tape (frozen statistics) stays fp32
        if K.native_fp16() and (train or not taping(input_layer, self.conv1.kernel, self.norm1.gamma)):
            x, d1 = self.d1(K.vgg_preprocess(il, 16, K.HALF))    # fp16 feature maps, 16 channels: the 16-channel MFMA tile
        else:
            # tape-free fp32 inference: the tail (below) uses d1's skip tensor only through a 64 -> 3 linear map, formed in the epilogue
            # of d1.conv2 where its planned kernel can do that -- the 64-channel full-resolution skip tensor is then never written
            if not train and K.PRECISION == "fp32" and not taping(input_layer, self.conv1.kernel, self.norm1.gamma):
                tail = self._tail_projection()
            if tail is not None:
                x, d1, d1_projected = self.d1(K.vgg_preprocess(il, 4), proj=tail["skip_map"])
            else:
                x, d1 = self.d1(K.vgg_preprocess(il, 4))   # same, zero 4th channel: MFMA-friendly
        x, d2 = self.d2(x)
        x, d3 = self.d3(x)
        x, d4 = self.d4(x)
        enc, d5 = self.d5(x)
        # data-parallel steps: the backward pass reaches this point when the gradients of every variable created after d5 (conv1,
        # norm1, the decoder, the skip layers: 60 of the net's 98 MB) are complete -- their all-reduce starts under the encoder's backward
        enc = K.mark(enc, getattr(self, "_decoder_grads_done", None))
        frozen = not train and taping(input_layer, self.conv1.kernel, self.norm1.gamma)
        if train:
            x = self.norm1.train_apply(self.conv1(enc), relu=True)
        elif frozen:
            x = self.norm1.frozen_apply(self.conv1(enc), relu=True)
        else:
            sc, sh = self.norm1.folded()
            x = self.conv1(enc, scale=sc, shift=sh, act2=K.ACT_RELU)   # conv -> BN -> relu (:163-165)
        x = self.s5(self.u5(x, training), d5)
        x = self.s4(self.u4(x, training), d4)
        x = self.s3(self.u3(x, training), d3)
        x = self.s2(self.u2(x, training), d2)
        if train or frozen:
            x = self.s1(self.u1(x, training), d1)
            if train:
                x = self.norm2.train_apply(self.conv2.call_padded(x, cout_pad=16), relu=True)
            else:
                x = self.norm2.frozen_apply(self.conv2.call_padded(x, cout_pad=16), relu=True)
        else:
            # inference: s1 (1x1 on concat[u1, d1 / 255], no activation: hallucination_net.py:179) and conv2 (1x1, :183) are two
            # linear maps in a row -- ONE 1x1 convolution 64 + 64 -> 3 with the composed filter W1 W2 and bias b1 W2 + b2 (a 128 x 3
            # matrix, composed in float64 once per parameter version).  The 64-channel full-resolution tensor between them (1 GB
            # written and read back at 16 x 512^2) never exists.
            sc, sh = self.norm2.folded()
            if d1_projected:
                # relu(sc (W_u u1 + W_d d1 / 255 + b) + sh) with both products as projections out of the producing kernels' epilogues
                # (sc folded into the maps): neither u1's nor d1's 64-channel tensor (1 GB each at 16 x 512^2) reaches HBM
                pu = self.u1.call_projected(x, tail["up_map"])
                if pu is not None:
                    x = K.affine_act(pu, shift=tail["const"], residual=d1, act=K.ACT_RELU)
                else:                                  # u1 on another kernel: its half of the composed 1x1 map as a convolution
                    x = K.conv2d(self.u1(x, training), tail["up_filter"], tail["bias"], cout_valid=3, scale=sc, shift=sh, residual=d1,
                                 act2=K.ACT_RELU)
            else:
                wc, bc = self._tail_filter(d1.shape[-1])
                x = K.conv2d(self.u1(x, training), wc, bc, x2=d1, cout_valid=3, scale=sc, shift=sh, act2=K.ACT_RELU)   # (:179-185)
        return self.s0(x, bgr, act1=K.ACT_RELU)                    # relu(s0(x, bgr)) (:188-190)

    def _tail_projection(self):
        """the composed tail (s1 -> conv2 -> folded norm2) split by source: [3, 64] maps for u1's and d1's 64 channels with norm2's scale
        folded in (the d1 map also carries the 1 / 255), the constant sc (b1 W2 + b2) + sh, and u1's half as a 1x1 filter for the
        fallback; cached per parameter version"""
        c_skip = self.s1.conv1.kernel.shape[2] - 64
        if c_skip != 64:
            return None
        wc, bc = self._tail_filter(c_skip)
        sc, sh = self.norm2.folded()
        n2 = self.norm2
        key = (self._tail[0], n2.gamma._version, n2.beta._version, n2.moving_mean._version, n2.moving_variance._version)
        if getattr(self, "_tail_proj", None) is None or self._tail_proj[0] != key:
            with torch.no_grad():
                m = wc[0, 0, :, :3] * sc[:3]                                   # [128, 3]
                up_filter = wc[:, :, :64, :].contiguous()
                up_filter._shdr_const = True
                self._tail_proj = (key, dict(up_map=m[:64].t().contiguous(), skip_map=m[64:].t().contiguous(),
                                             const=(sc[:3] * bc + sh[:3]).contiguous(), up_filter=up_filter, bias=bc),
                                   K.Ready(wc.device))
        self._tail_proj[2].wait()          # (built on the stream that asked first: K.Ready)
        return self._tail_proj[1]

    def _tail_filter(self, c_skip):
        """composed 1x1 filter [1,1,64 + c_skip,16] (3 real output channels) and bias [3] of s1 -> conv2; the skip rows carry the 1/255"""
        k1, b1, k2, b2 = self.s1.conv1.kernel, self.s1.conv1.bias, self.conv2.kernel, self.conv2.bias
        key = (k1._version, b1._version, k2._version, b2._version, c_skip)
        if getattr(self, "_tail", None) is None or self._tail[0] != key:
            with torch.no_grad():
                w1 = k1.detach().double().reshape(k1.shape[2], k1.shape[3]).clone()      # [128, 64]
                w1[w1.shape[0] - c_skip:] *= 1.0 / 255
                w2 = k2.detach().double().reshape(k2.shape[2], k2.shape[3])              # [64, 3]
                wc = torch.zeros((1, 1, w1.shape[0], 16), device=k1.device, dtype=torch.float32)
                wc[0, 0, :, :3] = (w1 @ w2).float()
                bc = (b1.detach().double() @ w2 + b2.detach().double()).float().contiguous()
                wc._shdr_const = True
            self._tail = (key, wc, bc, K.Ready(wc.device))
        self._tail[3].wait()               # (built on the stream that asked first: K.Ready)
        return self._tail[1], self._tail[2]
