// Front end of the training step (cfg.frontend): the host orchestration of the text encoder, the
// reference encoders, GST and the style-embedding losses, forward and backward.  The kernels it
// launches are train_front.hip's (through train_front.h), gemm.hip's and, through the launchers of
// train_ctx.h, train.hip's; the style-loss kernels are below.
#include <cmath>

#include "train_ctx.h"
#include "train_front.h"

namespace tt2 {

// ---- front end (cfg.frontend): encoder, reference encoders, GST in training mode -------------------
// The step starts from ids / reference mels: forward builds the memory the decoder slice consumes
// (tacotron.py:215-308), backward continues from the decoder's d memory (DMEM) into every front-end
// variable (train_front.hip kernels + gemm.hip products).
// conv layer scope of stack r in conv2d_i/: AdaIN's two stacks share 'refnet/conv2d_i' and
// tf.layers uniquifies the second (emotion) layer's default name (modules.py:84-87)
static std::string fe_ref_conv(const tt2_train_ctx* c, int r) { return c->f_adain && r == 0 ? "conv2d_1/" : "conv2d/"; }
// stride of refnet layer i: (2, 2) everywhere, AdaIN (2,2),(2,2),(1,1)x4 (tacotron.py:237)
static int fe_ref_stride(const tt2_train_ctx* c, int i) { return c->f_adain && i >= 2 ? 1 : 2; }
static std::string fe_mh_scope(int r) { return vn(r == 0 ? "Multihead-attention-emt/" : "Multihead-attention-spk/"); }
static std::string fe_lstm_scope(int d) {
  return vn(d == 0 ? "encoder_LSTM/bidirectional_rnn/fw/lstm_cell/" : "encoder_LSTM/bidirectional_rnn/bw/lstm_cell/");
}
static bool fe_regularized(const std::string& n) {  // tacotron.py:865-867 (oracle/train_ref.py regularized)
  return !(n.find("bias") != std::string::npos || n.find("Bias") != std::string::npos ||
           n.find("_projection") != std::string::npos || n.find("inputs_embedding") != std::string::npos ||
           n.find("RNN") != std::string::npos || n.find("LSTM") != std::string::npos);
}

void tr_front_build_vars(tt2_train_ctx* c,
                         const std::function<void(const std::string&, std::vector<int64_t>, bool)>& add) {
  const auto& f = c->cfg;
  const int E = f.embedding_dim, C = f.enc_conv_channels, K = f.enc_conv_kernel, U = f.encoder_lstm_units;
  auto addr = [&](const std::string& n, std::vector<int64_t> sh) { add(n, sh, fe_regularized(n)); };
  addr(vn("inputs_embedding"), {f.n_symbols, E});
  for (int i = 1; i <= f.enc_conv_layers; ++i) {
    const std::string s = fe_conv_scope(i);
    addr(s + "conv1d/kernel", {K, i == 1 ? E : C, C});
    addr(s + "conv1d/bias", {C});
    addr(s + "batch_normalization/gamma", {C});
    addr(s + "batch_normalization/beta", {C});
    add(s + "batch_normalization/moving_mean", {C}, false);
    add(s + "batch_normalization/moving_variance", {C}, false);
  }
  for (int d = 0; d < 2; ++d) {
    addr(fe_lstm_scope(d) + "kernel", {C + U, 4 * U});
    addr(fe_lstm_scope(d) + "bias", {4 * U});
  }
  const int RD = f.reference_depth, tokd = f.style_embed_depth / f.num_heads, A = f.style_att_dim, dh = A / f.num_heads;
  if (c->f_adain) {  // 'refnet' (modules.py:66-107): both conv stacks per layer, then GRU + dense
    const std::string rs = fe_ref_scope(c, 1);
    int ci = 1;
    for (int i = 0; i < 6; ++i) {
      const std::string s = rs + "conv2d_" + std::to_string(i) + "/";
      for (int r = 1; r >= 0; --r) {  // speaker stack first (conv2d/), then emotion (conv2d_1/)
        addr(s + fe_ref_conv(c, r) + "kernel", {3, 3, ci, f.reference_filters[i]});
        addr(s + fe_ref_conv(c, r) + "bias", {f.reference_filters[i]});
      }
      ci = f.reference_filters[i];
    }
    addr(rs + "rnn/gru_cell/gates/kernel", {c->f_gin + RD, 2 * RD});
    addr(rs + "rnn/gru_cell/gates/bias", {2 * RD});
    addr(rs + "rnn/gru_cell/candidate/kernel", {c->f_gin + RD, RD});
    addr(rs + "rnn/gru_cell/candidate/bias", {RD});
    addr(rs + "dense/kernel", {RD, 128});
    addr(rs + "dense/bias", {128});
    return;
  }
  for (int r = 0; r < c->f_nref; ++r) {
    const std::string rs = fe_ref_scope(c, r);
    int ci = 1;
    for (int i = 0; i < 6; ++i) {
      const std::string s = rs + "conv2d_" + std::to_string(i) + "/";
      addr(s + "conv2d/kernel", {3, 3, ci, f.reference_filters[i]});
      addr(s + "conv2d/bias", {f.reference_filters[i]});
      addr(s + "batch_normalization/gamma", {f.reference_filters[i]});
      addr(s + "batch_normalization/beta", {f.reference_filters[i]});
      add(s + "batch_normalization/moving_mean", {f.reference_filters[i]}, false);
      add(s + "batch_normalization/moving_variance", {f.reference_filters[i]}, false);
      ci = f.reference_filters[i];
    }
    addr(rs + "rnn/gru_cell/gates/kernel", {c->f_gin + RD, 2 * RD});
    addr(rs + "rnn/gru_cell/gates/bias", {2 * RD});
    addr(rs + "rnn/gru_cell/candidate/kernel", {c->f_gin + RD, RD});
    addr(rs + "rnn/gru_cell/candidate/bias", {RD});
    addr(rs + "dense/kernel", {RD, 128});
    addr(rs + "dense/bias", {128});
    if (!f.use_gst) continue;  // hp.use_gst = False: no style tokens / style attention (tacotron.py:284-291)
    addr(vn(r == 0 ? "style_tokens_emt" : "style_tokens_spk"), {f.num_gst, tokd});
    const std::string m = fe_mh_scope(r);
    addr(m + "conv1d/kernel", {1, 128, A});
    addr(m + "conv1d/bias", {A});
    addr(m + "conv1d_1/kernel", {1, tokd, A});
    addr(m + "conv1d_1/bias", {A});
    addr(m + "attention_v", {dh});
    addr(m + "attention_g", {});
    addr(m + "attention_b", {dh});
  }
  // Style_Emb_Disc dense layers (modules.py:626-644, tacotron.py:489-493; oracle style_disc_var_names)
  for (int r = 0; r < c->f_nref; ++r) {
    const int n = r == 0 ? f.n_emt : f.n_spk;
    if (n <= 0) continue;
    const std::string sd = vn(r == 0 ? "style_disc_emt/dense/" : "style_disc_spk/dense/");
    addr(sd + "kernel", {128, n});
    addr(sd + "bias", {n});
  }
}

// the encoder BiLSTM steps as fused products (k_tr_fused TF_EFWD / TF_EBWD): bf16 step, B <= 64,
// U a multiple of 128; TT2_TR_FUSED=0 keeps the split products + cell launches
static bool fe_enc_fused(const tt2_train_ctx* c) {
  const int U = c->cfg.encoder_lstm_units;
  return c->sw.fused && tr_prec(c) == 2 && c->B <= 64 && U % 128 == 0;
}

void tr_front_alloc(tt2_train_ctx* c) {
  const auto& f = c->cfg;
  const long B = c->B, T = c->Tin, C = f.enc_conv_channels, E = f.embedding_dim, U = f.encoder_lstm_units;
  const long BT = B * T, K = f.enc_conv_kernel;
  auto a = [](DevBuf& d, long n) { d.alloc(sizeof(float) * (size_t)std::max<long>(n, 1)); };
  a(c->fEX, BT * E);
  // one plane buffer serves the embedding (stride E) and the conv layers (stride C): the pad rows
  // are zeroed once per shape, so the two strides must agree or the stride-E frames land on the
  // stride-C pad rows (the im2col path serves E != C)
  // (TT2_PN_PLANES=0: the implicit-im2col gemm_x3_kernel convs here too)
  if (c->sw.pn_planes && c->cfg.precision && C % 64 == 0 && E == C && (K & 1) &&
      K <= 2 * CX_P + 1) {
    const long W = std::max(C, E), Wr = (W + 255) / 256 * 256;
    c->fePl.alloc((size_t)cx_rows((int)B, (int)T) * W * 2);
    c->feWt.alloc((size_t)Wr * K * W * 2);
  }
  for (int i = 0; i < f.enc_conv_layers; ++i) {
    a(c->fEA[i], BT * C);
    a(c->fEY[i + 1], BT * C);
  }
  a(c->fXP, BT * 8 * U); a(c->fGZ, 2 * B * 4 * U); a(c->fGA, 2 * T * B * 4 * U); a(c->fCN, 2 * T * B * U);
  a(c->fCS, 2 * (T + 1) * B * U); a(c->fHS, 2 * (T + 1) * B * U); a(c->fENC, BT * 2 * U);
  a(c->fMEM, BT * c->D); a(c->fSTY, B * (c->D - 2 * U)); a(c->fDSTY, B * (c->D - 2 * U));
  a(c->fDZ, 2 * T * B * 4 * U); a(c->fDHC, 2 * B * U); a(c->fDCC, 2 * B * U); a(c->fDHP, 2 * B * U);
  a(c->fdXP, BT * 8 * U); a(c->fdA, BT * std::max(C, E)); a(c->fdB, BT * std::max(C, E));
  a(c->fLWxT, 2 * 4 * U * C); a(c->fLWhT, 2 * 4 * U * U);
  {  // bf16 TF-layout operands of the fused encoder LSTM steps (k_tr_fused TF_EFWD / TF_EBWD)
    const long Bp = (B + 31) & ~31L;
    auto h = [](DevBuf& d, long n) { d.alloc(2 * (size_t)std::max<long>(n, 1)); };
    h(c->fTWf, 2 * 4 * U * U); h(c->fTWb, 2 * 4 * U * U); h(c->fHSh, 2 * (T + 1) * Bp * U); h(c->fDZh, 2 * 2 * Bp * 4 * U);
  }
  // reference encoders at max_T_ref
  const int RD = f.reference_depth, nm = c->NM;
  long fbuf = BT * K * std::max(C, E);  // encoder im2col^T
  // fDY / fDZc hold the refnet conv activations' gradients AND the encoder convs' BN backward
  // (dy, dz: B·T_in·C each)
  long mmax = BT * C;
  long wt_conv2d = 1;  // largest 3x3 conv2d kernel transpose [fo][9·ci]
  int H = f.max_T_ref, W = nm, ci = 1;
  for (int i = 0; i < 6; ++i) {
    const int st = fe_ref_stride(c, i), Ho = (H + st - 1) / st, Wo = (W + st - 1) / st, fo = f.reference_filters[i];
    const long M = B * Ho * Wo;
    for (int r = 0; r < c->f_nref; ++r) {
      a(c->fRA[r][i], c->f_adain ? 1 : M * fo);  // pre-BN activations (AdaIN: no batch norm)
      a(c->fRY[r][i], M * fo);
    }
    fbuf = std::max(fbuf, 9L * ci * M);
    mmax = std::max(mmax, std::max(M * fo, B * (long)H * W * ci));
    wt_conv2d = std::max(wt_conv2d, 9L * ci * fo);
    H = Ho; W = Wo; ci = fo;
  }
  const long T2 = H;
  c->f_T2max = (int)T2;
  // FB also holds the transposes of the GRU states / inputs over all T2·B rows and the BiLSTM states
  fbuf = std::max({fbuf, T2 * B * std::max<long>((long)W * ci, RD), BT * U, BT * C});
  for (int r = 0; r < c->f_nref; ++r) {
    a(c->fXG[r], B * T2 * 3 * RD); a(c->fGR[r], T2 * B * RD); a(c->fGU[r], T2 * B * RD); a(c->fGCC[r], T2 * B * RD);
    a(c->fGRH[r], T2 * B * RD); a(c->fHG[r], (T2 + 1) * B * RD); a(c->fREF[r], B * 128);
  }
  a(c->fGG, B * 2 * RD); a(c->fGC, B * RD);
  if (c->f_adain) {
    const long nmap = T2 * B * (long)W * ci;
    a(c->fADX, nmap); a(c->fDYE, std::max(mmax, nmap));
    a(c->fADM, 2L * B * ci * 2); a(c->fADS, (long)B * ci * 2);
    mmax = std::max(mmax, nmap);
  }
  a(c->fFBUF, fbuf); a(c->fDY, mmax); a(c->fDY2, mmax); a(c->fDZc, mmax);
  // the direct conv2d kernel gradient sums its partial rows with tr_colsum over 9·ci·fo columns
  c->part.reserve(sizeof(float) * (size_t)(wt_conv2d + 4096));
  const int ntok = f.num_gst, tokd = f.style_embed_depth / f.num_heads, A = f.style_att_dim, dh = A / f.num_heads;
  a(c->fGq, B * A); a(c->fGkk, B * ntok * A); a(c->fGv, B * ntok * tokd); a(c->fGnv, B * dh); a(c->fGbb, B * dh);
  a(c->fGsum, ntok * A + ntok * tokd + 2 * dh);
  a(c->sXREF, 2 * B * 128); a(c->sDL, B * std::max(1, std::max(f.n_emt, f.n_spk))); a(c->sOM, B * B);
  c->sLAB.alloc(sizeof(int) * (size_t)(2 * B));
  a(c->fdREF, B * 128); a(c->fDZD, B * 128); a(c->fDH, B * RD); a(c->fDHA, B * RD); a(c->fDRH, B * RD);
  a(c->fDCP, T2 * B * RD); a(c->fDGP, T2 * B * 2 * RD); a(c->fDXG, B * T2 * 3 * RD);
  // transposed / flipped weight scratch: refnet conv2d kernels, GRU gates + candidate, dense, GST
  // query, and the encoder conv flip K·cin·C with cin = E for the first layer
  a(c->fWT, std::max<long>({wt_conv2d, 3L * RD * std::max<long>(c->f_gin, RD), 128L * RD, 128L * A,
                            (long)K * std::max(C, E) * C}));
  a(c->fBN, 2L * (f.enc_conv_layers + 6 * c->f_nref) * 512);
  a(c->fpart, 64L * 2 * 512 + 1024);
}

// batch statistics over M rows of [M][C] into mean / var (k_pn_colstat: biased variance)
static void fe_stats(tt2_train_ctx* c, const float* x, long M, int C, float* mean, float* var, hipStream_t s) {
  tr_bn_stats(x, M, C, 64L * 512, c->fpart.as<float>(), mean, var, s);
}
// BN backward (batch statistics) from dy -> dz (act: 0 none, 2 relu' from the pre-BN activation)
static void fe_bn_bwd(tt2_train_ctx* c, const float* dxn, const uint8_t* keep, const float* a, long M, int C,
                      const float* mean, const float* var, const std::string& sc, int act, float* dy, float* dz,
                      hipStream_t s, __bf16* planes = nullptr, int T = 1) {
  float* part = c->fpart.as<float>();
  tr_bn_bwd(dxn, keep, a, M, C, mean, var, c->cfg.bn_eps, pvar(c, sc + "batch_normalization/gamma"),
            gvar(c, sc + "batch_normalization/gamma"), gvar(c, sc + "batch_normalization/beta"), 64L * 512, part,
            part + 64L * 2 * 512, act, dy, dz, planes, T, s);
}

// fp32 rows [B·T][C] (batch-major) -> the padded bf16 planes of conv_bf16_planes (frame rows only)
__global__ void k_rows_to_planes(const float* __restrict__ x, long M, int C, int T, __bf16* __restrict__ planes) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M * C) pn_plane_put(planes, T, i, C, x[i]);
}

static FeGst fe_gst_args(tt2_train_ctx* c, int r, int B) {
  const auto& f = c->cfg;
  const std::string m = fe_mh_scope(r);
  FeGst g{};
  g.ref = c->fREF[r].as<float>();
  g.tokens = pvar(c, vn(r == 0 ? "style_tokens_emt" : "style_tokens_spk"));
  g.wq = pvar(c, m + "conv1d/kernel"); g.bq = pvar(c, m + "conv1d/bias");
  g.wk = pvar(c, m + "conv1d_1/kernel"); g.bk = pvar(c, m + "conv1d_1/bias");
  g.v = pvar(c, m + "attention_v"); g.g = pvar(c, m + "attention_g"); g.bb = pvar(c, m + "attention_b");
  g.N = B; g.ntok = f.num_gst; g.tokd = f.style_embed_depth / f.num_heads; g.A = f.style_att_dim; g.heads = f.num_heads;
  g.refd = 128;
  g.style = c->fSTY.as<float>(); g.style_ld = c->D - 2 * f.encoder_lstm_units; g.style_off = r * f.style_embed_depth;
  g.dstyle = c->fDSTY.as<float>();
  g.dq = c->fGq.as<float>(); g.pdkk = c->fGkk.as<float>(); g.pdv = c->fGv.as<float>(); g.pdnv = c->fGnv.as<float>();
  g.pdbb = c->fGbb.as<float>();
  return g;
}

void tr_front_forward(tt2_train_ctx* c, const int* ids, const int* lens, const float* const* refs, int T_ref,
                             const uint8_t* encm, const uint8_t* enczm, int T, hipStream_t s) {
  const auto& f = c->cfg;
  const int B = c->B, E = f.embedding_dim, C = f.enc_conv_channels, K = f.enc_conv_kernel, U = f.encoder_lstm_units;
  const long M = (long)B * T;
  const float eps = f.bn_eps;
  float* BN = c->fBN.as<float>();
  fe_embed(ids, pvar(c, vn("inputs_embedding")), M, E, c->fEX.as<float>(), s);
  // EncoderConvolutions (modules.py:251-280, conv1d() :485-497 with bnorm 'after'): conv -> ReLU ->
  // BN (batch statistics over all B·T positions) -> dropout(0.5, keep bits)
  // bf16 conv over padded planes (conv_bf16_planes, as the Postnet's): planes of the embedding here,
  // of each layer's output from its BN forward; pad rows zeroed once per shape
  const bool planes = c->fePl.p && tr_prec(c) == 2;
  __bf16* pl = reinterpret_cast<__bf16*>(c->fePl.p);
  __bf16* wt = reinterpret_cast<__bf16*>(c->feWt.p);
  if (planes) {
    if (c->fe_pl_B != B || c->fe_pl_T != T) {
      TT2_HIP(hipMemsetAsync(c->fePl.p, 0, c->fePl.bytes, s));
      c->fe_pl_B = B;
      c->fe_pl_T = T;
    }
    hipLaunchKernelGGL(k_rows_to_planes, dim3(nblk(M * E)), dim3(256), 0, s, c->fEX.as<float>(), M, E, T, pl);
  }
  for (int i = 0; i < f.enc_conv_layers; ++i) {
    const std::string sc = fe_conv_scope(i + 1);
    const int cin = i == 0 ? E : C;
    if (planes) {
      kc_transpose_bf16(pvar(c, sc + "conv1d/kernel"), K * cin, C, C, wt, K * cin, (C + 255) / 256 * 256, s);
      conv_bf16_planes(pl, cin, B, T, K, wt, (long)K * cin, C, pvar(c, sc + "conv1d/bias"), ACT_RELU,
                       c->fEA[i].as<float>(), C, s);
    } else {
      GemmArgs g;
      g.a_mode = A_CONV1D; g.M = (int)M; g.N = C; g.T = T; g.kw = K; g.pad = (K - 1) / 2; g.C = cin;
      g.A = i == 0 ? c->fEX.as<float>() : c->fEY[i].as<float>(); g.xs_b = (long)T * cin; g.xs_t = cin; g.K = K * cin;
      g.Bw = pvar(c, sc + "conv1d/kernel"); g.ldb = C; g.Cout = c->fEA[i].as<float>(); g.ldc = C;
      g.bias = pvar(c, sc + "conv1d/bias"); g.act = ACT_RELU;
      tr_gemm_run(c, g, s);
    }
    float* mean = BN + (long)i * 2 * 512;
    float* var = mean + 512;
    fe_stats(c, c->fEA[i].as<float>(), M, C, mean, var, s);
    tr_bn_fwd(c->fEA[i].as<float>(), M, C, mean, var, pvar(c, sc + "batch_normalization/gamma"),
              pvar(c, sc + "batch_normalization/beta"), eps, encm ? encm + (long)i * M * C : nullptr,
              c->fEY[i + 1].as<float>(), planes && i + 1 < f.enc_conv_layers ? pl : nullptr, T, s);
  }
  // EncoderRNN (modules.py:283-323): input projections of both directions for every position
  const float* X = c->fEY[f.enc_conv_layers].as<float>();
  for (int d = 0; d < 2; ++d)
    tr_gemm(c, (int)M, 4 * U, C, X, C, pvar(c, fe_lstm_scope(d) + "kernel"), 4 * U, c->fXP.as<float>() + d * 4 * U, 8 * U,
            s, pvar(c, fe_lstm_scope(d) + "bias"));
  TT2_HIP(hipMemsetAsync(c->fENC.p, 0, sizeof(float) * (size_t)M * 2 * U, s));
  for (int d = 0; d < 2; ++d) {  // zero initial states
    TT2_HIP(hipMemsetAsync(c->fCS.as<float>() + (long)d * (T + 1) * B * U, 0, sizeof(float) * (size_t)B * U, s));
    TT2_HIP(hipMemsetAsync(c->fHS.as<float>() + (long)d * (T + 1) * B * U, 0, sizeof(float) * (size_t)B * U, s));
  }
  FeLstm l{};
  l.XP = c->fXP.as<float>(); l.GZ = c->fGZ.as<float>(); l.GA = c->fGA.as<float>(); l.CN = c->fCN.as<float>();
  l.CS = c->fCS.as<float>(); l.HS = c->fHS.as<float>(); l.ENC = c->fENC.as<float>(); l.zm = enczm; l.lens = lens;
  l.B = B; l.T = T; l.U = U; l.zo = f.zoneout;
  if (fe_enc_fused(c)) {  // both directions' recurrent product + cell in one launch per step
    const long Bp = (B + 31) & ~31L;
    for (int d = 0; d < 2; ++d)
      tr_tf_weights_f32(pvar(c, fe_lstm_scope(d) + "kernel") + (long)C * 4 * U, (long)4 * U, 1, 4 * U, U, U / 8,
                        (int)TF_EFWD, U, c->fTWf.as<__bf16>() + (long)d * 4 * U * U, s);
    for (int d = 0; d < 2; ++d)  // zero initial h
      TT2_HIP(hipMemsetAsync(c->fHSh.as<__bf16>() + (long)d * (T + 1) * Bp * U, 0, 2 * (size_t)Bp * U, s));
    TrFused e{};
    e.Wt = c->fTWf.as<__bf16>(); e.wdir = (long)4 * U * U; e.K = U; e.B = B; e.H = U; e.T = T; e.lens = lens;
    e.zm = enczm; e.zo = f.zoneout; e.XP = c->fXP.as<float>(); e.GA = c->fGA.as<float>(); e.CN = c->fCN.as<float>();
    e.CS = c->fCS.as<float>(); e.HS = c->fHS.as<float>(); e.ENC = c->fENC.as<float>(); e.HSh = c->fHSh.as<__bf16>();
    e.adir = (T + 1) * Bp * U;
    for (int t = 0; t < T; ++t) {
      e.t = t;
      tr_fused_enc_step(e, false, s);
    }
  } else {
    for (int t = 0; t < T; ++t) {
      for (int d = 0; d < 2; ++d)
        tr_gemm(c, B, 4 * U, U, c->fHS.as<float>() + ((long)d * (T + 1) + t) * B * U, U,
                pvar(c, fe_lstm_scope(d) + "kernel") + (long)C * 4 * U, 4 * U, c->fGZ.as<float>() + (long)d * B * 4 * U,
                4 * U, s);
      l.t = t;
      fe_lstm_cell(l, s);
    }
  }
  // reference encoders (modules.py:9-64) + GST (tacotron.py:276-282)
  const int RD = f.reference_depth;
  int nbn = f.enc_conv_layers;
  for (int r = 0; r < c->f_nref; ++r) {
    const std::string rs = fe_ref_scope(c, r);
    int H = T_ref, W = c->NM, ci = 1;
    const float* x = refs[r];
    for (int i = 0; i < 6; ++i) {
      const std::string sc = rs + "conv2d_" + std::to_string(i) + "/";
      const int st = fe_ref_stride(c, i);
      const int fo = f.reference_filters[i], Ho = (H + st - 1) / st, Wo = (W + st - 1) / st;
      GemmArgs g;
      g.M = B * Ho * Wo; g.N = fo; g.K = 9 * ci; g.a_mode = A_CONV2D; g.A = x;
      g.H = H; g.Wd = W; g.C = ci; g.Ho = Ho; g.Wo = Wo; g.kh = 3; g.kw2 = 3; g.sh = st; g.sw = st;
      g.pt = std::max((Ho - 1) * st + 3 - H, 0) / 2; g.pl = std::max((Wo - 1) * st + 3 - W, 0) / 2;
      g.Bw = pvar(c, sc + fe_ref_conv(c, r) + "kernel"); g.ldb = fo; g.ldc = fo;
      g.bias = pvar(c, sc + fe_ref_conv(c, r) + "bias");
      const bool small = c->sw.fe_direct && fe_conv2d_fwd_small_ok(ci, fo);  // first layer: direct kernel
      if (c->f_adain) {  // conv2d(..., batch_norm=False): conv + ReLU (modules.py:84-87)
        g.Cout = c->fRY[r][i].as<float>();
        g.act = ACT_RELU;
        if (small)
          fe_conv2d_fwd_small(x, g.Bw, g.bias, B, H, W, ci, Ho, Wo, fo, g.pt, g.pl, st, true, g.Cout, s, tr_prec(c) == 2);
        else
          tr_gemm_run(c, g, s);
      } else {
        g.Cout = c->fRA[r][i].as<float>();
        if (small)
          fe_conv2d_fwd_small(x, g.Bw, g.bias, B, H, W, ci, Ho, Wo, fo, g.pt, g.pl, st, false, g.Cout, s, tr_prec(c) == 2);
        else
          tr_gemm_run(c, g, s);
        float* mean = BN + (long)nbn * 2 * 512;
        float* var = mean + 512;
        fe_stats(c, c->fRA[r][i].as<float>(), g.M, fo, mean, var, s);
        fe_bn_relu_fwd(c->fRA[r][i].as<float>(), g.M, fo, mean, var, pvar(c, sc + "batch_normalization/gamma"),
                       pvar(c, sc + "batch_normalization/beta"), eps, c->fRY[r][i].as<float>(), s);
        ++nbn;
      }
      x = c->fRY[r][i].as<float>();
      H = Ho; W = Wo; ci = fo;
    }
    const int T2 = H, gin = W * ci;
    c->f_T2 = T2;
    if (c->f_adain) {
      // moments over (time, freq) per row and channel (modules.py:90-91); the speaker map (r = 1,
      // after the emotion stack r = 0) restyled into fADX, which alone feeds the GRU (:94-104)
      float* mv = c->fADM.as<float>() + (long)r * B * ci * 2;
      fe_ad_moments(x, B, T2 * W, ci, mv, s);
      if (r == 0) continue;
      fe_ad_mix(x, B, T2 * W, ci, mv, c->fADM.as<float>(), c->fADX.as<float>(), s);
      x = c->fADX.as<float>();
    }
    const float* kg = pvar(c, rs + "rnn/gru_cell/gates/kernel");
    const float* kcn = pvar(c, rs + "rnn/gru_cell/candidate/kernel");
    float* XG = c->fXG[r].as<float>();
    tr_gemm(c, B * T2, 2 * RD, gin, x, gin, kg, 2 * RD, XG, 3 * RD, s, pvar(c, rs + "rnn/gru_cell/gates/bias"));
    tr_gemm(c, B * T2, RD, gin, x, gin, kcn, RD, XG + 2 * RD, 3 * RD, s, pvar(c, rs + "rnn/gru_cell/candidate/bias"));
    TT2_HIP(hipMemsetAsync(c->fHG[r].p, 0, sizeof(float) * (size_t)B * RD, s));
    if (c->sw.fe_gru_seq && fe_gru_seq_ok(B, RD))  // the whole recurrence in one work-group (fp32 MFMA)
      fe_gru_fwd_seq(XG, kg + (long)gin * 2 * RD, kcn + (long)gin * RD, B, T2, RD, c->fGR[r].as<float>(), c->fGU[r].as<float>(),
                     c->fGRH[r].as<float>(), c->fGCC[r].as<float>(), c->fHG[r].as<float>(), s, tr_prec(c) == 2);
    for (int t = 0; t < (c->sw.fe_gru_seq && fe_gru_seq_ok(B, RD) ? 0 : T2); ++t) {
      float* h = c->fHG[r].as<float>() + (long)t * B * RD;
      tr_gemm(c, B, 2 * RD, RD, h, RD, kg + (long)gin * 2 * RD, 2 * RD, c->fGG.as<float>(), 2 * RD, s);
      fe_gru_a(XG, c->fGG.as<float>(), c->fHG[r].as<float>(), B, T2, RD, t, c->fGR[r].as<float>(),
               c->fGU[r].as<float>(), c->fGRH[r].as<float>(), s);
      tr_gemm(c, B, RD, RD, c->fGRH[r].as<float>() + (long)t * B * RD, RD, kcn + (long)gin * RD, RD, c->fGC.as<float>(), RD,
              s);
      fe_gru_b(XG, c->fGC.as<float>(), c->fGU[r].as<float>(), B, T2, RD, t, c->fGCC[r].as<float>(),
               c->fHG[r].as<float>(), s);
    }
    tr_gemm(c, B, 128, RD, c->fHG[r].as<float>() + (long)T2 * B * RD, RD, pvar(c, rs + "dense/kernel"), 128,
            c->fREF[r].as<float>(), 128, s, pvar(c, rs + "dense/bias"), nullptr, 0, ACT_TANH);
    if (c->f_adain) {  // the speaker reference embedding is the style embedding (tacotron.py:269-272)
      tr_rows_copy(c->fREF[r].as<float>(), 128L, (long)B, 128, c->fSTY.as<float>(),
                   (long)(c->D - 2 * f.encoder_lstm_units), nullptr, 0L, s);
    } else if (f.use_gst) {
      fe_gst_fwd(fe_gst_args(c, r, B), s);
    } else {  // the reference embedding is the style embedding (tacotron.py:284-291)
      const int SW = c->D - 2 * f.encoder_lstm_units;
      tr_rows_copy(c->fREF[r].as<float>(), 128L, (long)B, 128, c->fSTY.as<float>() + r * 128, (long)SW, nullptr, 0L, s);
    }
  }
  fe_memory(c->fENC.as<float>(), c->fSTY.as<float>(), B, T, 2 * U, c->D - 2 * U, c->fMEM.as<float>(), s);
  c->f_ran = true;
}

// ---- style-embedding losses (tacotron.py:486-495, 812-820, 840-846; oracle style_emb_losses) ----------
// Style_Emb_Disc: logits = ref·W + b [B, n]; softmax_cross_entropy_with_logits against tf.one_hot(label)
// (out-of-range label: zero row -> loss 0, gradient 0), batch mean.  One work-group per row: the
// row's loss -> part[b], d logits = (softmax·Σy - y) / B -> DL, d ref += DL·Wᵀ -> XR.
__global__ __launch_bounds__(128) void k_fe_disc(const float* __restrict__ ref, const float* __restrict__ Wk,
                                                 const float* __restrict__ bk, const int* __restrict__ lab, int B,
                                                 int n, float* __restrict__ DL, float* __restrict__ XR,
                                                 float* __restrict__ part) {
  extern __shared__ float sd[];  // [128] ref row, [n] logits
  const int b = blockIdx.x, k = threadIdx.x;
  float* lg = sd + 128;
  sd[k] = ref[(long)b * 128 + k];
  __syncthreads();
  for (int j = k; j < n; j += 128) {
    float v = bk[j];
    for (int i = 0; i < 128; ++i) v = fmaf(sd[i], Wk[(long)i * n + j], v);
    lg[j] = v;
  }
  __syncthreads();
  const int y = lab[b];
  const bool hot = y >= 0 && y < n;
  if (k == 0) {  // serial over n (small): max, log-sum-exp, loss
    float mx = -INFINITY;
    for (int j = 0; j < n; ++j) mx = fmaxf(mx, lg[j]);
    double se = 0;
    for (int j = 0; j < n; ++j) se += exp((double)(lg[j] - mx));
    const float lse = mx + (float)log(se);
    part[b] = hot ? lse - lg[y] : 0.f;
    sd[128 + n] = lse;
  }
  __syncthreads();
  const float lse = sd[128 + n];
  for (int j = k; j < n; j += 128) {
    const float d = hot ? (expf(lg[j] - lse) - (j == y ? 1.f : 0.f)) / (float)B : 0.f;
    DL[(long)b * n + j] = d;
    lg[j] = d;
  }
  __syncthreads();
  float g = 0.f;
  for (int j = 0; j < n; ++j) g = fmaf(lg[j], Wk[(long)k * n + j], g);
  XR[(long)b * 128 + k] += g;
}
// d W[k][j] = Σ_b ref[b][k] DL[b][j], d b[j] = Σ_b DL[b][j] (written, not accumulated)
__global__ void k_fe_disc_wgrad(const float* __restrict__ ref, const float* __restrict__ DL, int B, int n,
                                float* __restrict__ dW, float* __restrict__ db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 128 * n) {
    const int k = i / n, j = i % n;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v = fmaf(ref[(long)b * 128 + k], DL[(long)b * n + j], v);
    dW[i] = v;
  } else if (i < 129 * n) {
    const int j = i - 128 * n;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += DL[(long)b * n + j];
    db[j] = v;
  }
}
// orthogonality loss w·||E·Sᵀ||_F: M = E·Sᵀ [B][B] (row b per work-group), Σ M² partials
__global__ __launch_bounds__(128) void k_fe_orthog_m(const float* __restrict__ E, const float* __restrict__ S, int B,
                                                     float* __restrict__ M, float* __restrict__ part) {
  __shared__ float e[128];
  __shared__ float s4[4];
  const int b = blockIdx.x, t = threadIdx.x;
  e[t] = E[(long)b * 128 + t];
  __syncthreads();
  float sq = 0.f;
  for (int jj = t; jj < B; jj += 128) {
    float v = 0.f;
    for (int i = 0; i < 128; ++i) v = fmaf(e[i], S[(long)jj * 128 + i], v);
    M[(long)b * B + jj] = v;
    sq += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  if ((t & 63) == 0) s4[t >> 6] = sq;
  __syncthreads();
  if (t == 0) part[b] = s4[0] + s4[1];
}
// loss = w·||M|| -> red[0]; d E = (w/||M||)·M·S -> XE, d S = (w/||M||)·Mᵀ·E -> XS (accumulated);
// blocks [0, B) rows of d E, [B, 2B) rows of d S.  ||M|| = 0: TF's norm gradient is NaN there; 0 here.
__global__ __launch_bounds__(128) void k_fe_orthog_g(const float* __restrict__ E, const float* __restrict__ S,
                                                     const float* __restrict__ M, int B, float w,
                                                     const float* __restrict__ n2, float* __restrict__ red,
                                                     float* __restrict__ XE, float* __restrict__ XS) {
  const int r = blockIdx.x, k = threadIdx.x;
  const float nrm = sqrtf(n2[0]);
  if (r == 0 && k == 0) red[0] = w * nrm;
  const float coef = nrm > 0.f ? w / nrm : 0.f;
  float g = 0.f;
  if (r < B) {
    for (int j = 0; j < B; ++j) g = fmaf(M[(long)r * B + j], S[(long)j * 128 + k], g);
    XE[(long)r * 128 + k] += coef * g;
  } else {
    const int j = r - B;
    for (int b = 0; b < B; ++b) g = fmaf(M[(long)b * B + j], E[(long)b * 128 + k], g);
    XS[(long)j * 128 + k] += coef * g;
  }
}

// The style-embedding losses' gradients into the refnet outputs (sXREF[r]) and the classifier
// weights; losses -> red[5] (emt), red[6] (spk), red[7] (orthogonality).  Before the refnet backward.
static void tr_style_losses(tt2_train_ctx* c, hipStream_t s) {
  const auto& f = c->cfg;
  const int B = c->B;
  float* red = c->red.as<float>();
  float* XR = c->sXREF.as<float>();
  TT2_HIP(hipMemsetAsync(XR, 0, sizeof(float) * (size_t)2 * B * 128, s));
  TT2_HIP(hipMemsetAsync(red + 5, 0, sizeof(float) * 3, s));
  for (int r = 0; r < c->f_nref; ++r) {
    const int n = r == 0 ? f.n_emt : f.n_spk;
    if (n <= 0) continue;
    const std::string sd = vn(r == 0 ? "style_disc_emt/dense/" : "style_disc_spk/dense/");
    hipLaunchKernelGGL(k_fe_disc, dim3(B), dim3(128), sizeof(float) * (129 + n), s, c->fREF[r].as<float>(),
                       pvar(c, sd + "kernel"), pvar(c, sd + "bias"), c->sLAB.as<int>() + r * B, B, n, c->sDL.as<float>(),
                       XR + (long)r * B * 128, c->part.as<float>());
    tr_sum_final(c->part.as<float>(), B, 1.0f / B, red + 5 + r, 0, s);
    hipLaunchKernelGGL(k_fe_disc_wgrad, dim3((129 * n + 255) / 256), dim3(256), 0, s, c->fREF[r].as<float>(),
                       c->sDL.as<float>(), B, n, gvar(c, sd + "kernel"), gvar(c, sd + "bias"));
  }
  if (f.orthog_weight > 0.f && c->f_nref == 2) {
    hipLaunchKernelGGL(k_fe_orthog_m, dim3(B), dim3(128), 0, s, c->fREF[0].as<float>(), c->fREF[1].as<float>(), B,
                       c->sOM.as<float>(), c->part.as<float>());
    tr_sum_final(c->part.as<float>(), B, 1.0f, red + 8, 0, s);
    hipLaunchKernelGGL(k_fe_orthog_g, dim3(2 * B), dim3(128), 0, s, c->fREF[0].as<float>(), c->fREF[1].as<float>(),
                       c->sOM.as<float>(), B, f.orthog_weight, red + 8, red + 7, XR, XR + (long)B * 128);
  }
  TT2_HIP(hipGetLastError());
}

bool tr_style_on(const tt2_train_ctx* c) {
  return c->cfg.n_emt > 0 || (c->f_nref == 2 && (c->cfg.n_spk > 0 || c->cfg.orthog_weight > 0.f));
}

void tr_front_backward(tt2_train_ctx* c, const int* ids, const int* lens, const float* const* refs, int T_ref,
                              const uint8_t* encm, const uint8_t* enczm, int T, hipStream_t s) {
  const auto& f = c->cfg;
  const int B = c->B, E = f.embedding_dim, C = f.enc_conv_channels, K = f.enc_conv_kernel, U = f.encoder_lstm_units;
  const int D = c->D, RD = f.reference_depth, SW = D - 2 * U;
  const long M = (long)B * T;
  float* BN = c->fBN.as<float>();
  float* WT = c->fWT.as<float>();
  float* FB = c->fFBUF.as<float>();
  // memory assembly: style gradient = Σ_t over the (length-masked) d memory rows
  fe_style_grad(c->DMEM.as<float>(), B, T, D, 2 * U, c->fDSTY.as<float>(), s);
  const bool style_on = tr_style_on(c);
  if (style_on) tr_style_losses(c, s);
  // conv2d stack r backward from d map `din` (conv -> BN -> ReLU per layer; AdaIN: conv -> ReLU)
  const bool fe_direct = c->sw.fe_direct;
  auto conv_bwd = [&](int r, const float* din) {
    const std::string rs = fe_ref_scope(c, r);
    float* dY = c->fDY.as<float>();
    int dims[7][3];
    {
      int H = T_ref, W = c->NM, ci = 1;
      for (int i = 0; i < 6; ++i) {
        dims[i][0] = H; dims[i][1] = W; dims[i][2] = ci;
        const int st = fe_ref_stride(c, i);
        H = (H + st - 1) / st; W = (W + st - 1) / st; ci = f.reference_filters[i];
      }
      dims[6][0] = H; dims[6][1] = W; dims[6][2] = ci;
    }
    for (int i = 5; i >= 0; --i) {
      const int nbn = f.enc_conv_layers + 6 * r + i;  // forward order: encoder convs, then refnet r's layers
      const std::string sc = rs + "conv2d_" + std::to_string(i) + "/", ly = fe_ref_conv(c, r);
      const int H = dims[i][0], W = dims[i][1], ci = dims[i][2], Ho = dims[i + 1][0], Wo = dims[i + 1][1];
      const int fo = f.reference_filters[i], st = fe_ref_stride(c, i);
      const long Mi = (long)B * Ho * Wo;
      float* dYr = c->fDY2.as<float>();
      fe_relu_mask(i == 5 ? din : dY, c->fRY[r][i].as<float>(), Mi * fo, dYr, s);
      float* dz = dYr;
      if (!c->f_adain) {
        const float* mean = BN + (long)nbn * 2 * 512;
        const float* var = mean + 512;
        dz = c->fDZc.as<float>();
        fe_bn_bwd(c, dYr, nullptr, c->fRA[r][i].as<float>(), Mi, fo, mean, var, sc, 0, dYr, dz, s);
      }
      tr_colsum(c, dz, Mi, fo, fo, gvar(c, sc + ly + "bias"), s);
      const int pt = std::max((Ho - 1) * st + 3 - H, 0) / 2, pl = std::max((Wo - 1) * st + 3 - W, 0) / 2;
      const float* xin = i == 0 ? refs[r] : c->fRY[r][i - 1].as<float>();
      // kernel gradient: direct (k_fe_conv2d_dw: patches staged in LDS, fp32 FMA, partial rows summed
      // by tr_colsum) where its register / LDS budget takes the channel counts, else the im2colᵀ
      // columns + GEMM (gemm_bf16_kc with the im2colᵀ gathered into bf16 measured 458 us per layer
      // against 525 + ~60 for the fp32 columns + gemm_x3_kernel: its 256-wide N tile is 8x idle at fo = 32)
      if (fe_direct && fe_conv2d_dw_ok(ci, fo)) {
        const int rows = fe_conv2d_dw(xin, dz, B, H, W, ci, Ho, Wo, fo, pt, pl, st, FB, (long)(c->fFBUF.bytes / sizeof(float)),
                                      s);
        tr_colsum(c, FB, rows, 9 * ci * fo, 9L * ci * fo, gvar(c, sc + ly + "kernel"), s);
      } else {
        fe_im2col2d_t(xin, B, H, W, ci, Ho, Wo, pt, pl, FB, Mi, s, st);
        tr_gemm(c, 9 * ci, fo, (int)Mi, FB, Mi, dz, fo, gvar(c, sc + ly + "kernel"), fo, s);
      }
      if (i > 0) {
        if (fe_direct && fe_conv2d_dx_ok(ci, W, Ho, Wo, fo, st)) {  // input gradient as a gather over the taps (k_fe_conv2d_dx)
          fe_conv2d_dx(dz, pvar(c, sc + ly + "kernel"), B, H, W, ci, Ho, Wo, fo, pt, pl, st, dY, s);
        } else {
          tr_transpose(pvar(c, sc + ly + "kernel"), 9L * ci, fo, fo, WT, 9L * ci, s);  // [fo][9ci]
          tr_gemm(c, (int)Mi, 9 * ci, fo, dz, fo, WT, 9 * ci, FB, 9 * ci, s);
          fe_col2im2d(FB, B, H, W, ci, Ho, Wo, pt, pl, dY, s, st);
        }
      }
    }
  };
  for (int r = c->f_adain ? 1 : 0; r < c->f_nref; ++r) {
    const std::string rs = fe_ref_scope(c, r), m = fe_mh_scope(r);
    if (!f.use_gst || c->f_adain) {  // d ref = d style slice (+ style-loss terms)
      tr_rows_copy(c->fDSTY.as<float>() + (c->f_adain ? 0 : r * 128), (long)SW, (long)B, 128, c->fdREF.as<float>(),
                   128L, style_on ? c->sXREF.as<float>() + (long)r * B * 128 : nullptr, 128L, s);
    } else {
    const FeGst ga = fe_gst_args(c, r, B);
    fe_gst_bwd(ga, s);
    const int ntok = ga.ntok, tokd = ga.tokd, A = ga.A, dh = A / ga.heads;
    float* sum = c->fGsum.as<float>();
    tr_colsum(c, ga.pdkk, B, ntok * A, (long)ntok * A, sum, s);
    tr_colsum(c, ga.pdv, B, ntok * tokd, (long)ntok * tokd, sum + ntok * A, s);
    tr_colsum(c, ga.pdnv, B, dh, dh, sum + ntok * A + ntok * tokd, s);
    tr_colsum(c, ga.pdbb, B, dh, dh, sum + ntok * A + ntok * tokd + dh, s);
    fe_gst_final(ga, sum, sum + ntok * A, sum + ntok * A + ntok * tokd, sum + ntok * A + ntok * tokd + dh,
                 gvar(c, m + "conv1d_1/kernel"), gvar(c, m + "conv1d_1/bias"),
                 gvar(c, vn(r == 0 ? "style_tokens_emt" : "style_tokens_spk")), gvar(c, m + "attention_v"),
                 gvar(c, m + "attention_g"), gvar(c, m + "attention_b"), s);
    // query conv1d (1x1): d Wq = refᵀ dq, d bq, d ref = dq Wqᵀ
    tr_transpose(c->fREF[r].as<float>(), B, 128, 128, WT, B, s);
    tr_gemm(c, 128, A, B, WT, B, ga.dq, A, gvar(c, m + "conv1d/kernel"), A, s);
    tr_colsum(c, ga.dq, B, A, A, gvar(c, m + "conv1d/bias"), s);
    tr_transpose(pvar(c, m + "conv1d/kernel"), 128, A, A, WT, 128, s);
    tr_gemm(c, B, 128, A, ga.dq, A, WT, 128, c->fdREF.as<float>(), 128, s, nullptr,
            style_on ? c->sXREF.as<float>() + (long)r * B * 128 : nullptr, 128);  // + style-loss terms
    }
    // dense tanh (modules.py:63)
    fe_tanh_bwd(c->fdREF.as<float>(), c->fREF[r].as<float>(), (long)B * 128, c->fDZD.as<float>(), s);
    const int T2 = c->f_T2;
    const float* hT = c->fHG[r].as<float>() + (long)T2 * B * RD;
    tr_transpose(hT, B, RD, RD, WT, B, s);
    tr_gemm(c, RD, 128, B, WT, B, c->fDZD.as<float>(), 128, gvar(c, rs + "dense/kernel"), 128, s);
    tr_colsum(c, c->fDZD.as<float>(), B, 128, 128, gvar(c, rs + "dense/bias"), s);
    tr_transpose(pvar(c, rs + "dense/kernel"), RD, 128, 128, WT, RD, s);
    tr_gemm(c, B, RD, 128, c->fDZD.as<float>(), 128, WT, RD, c->fDH.as<float>(), RD, s);
    // GRU BPTT (TF1 GRUCell): recurrent weight transposes once
    const int gin = c->f_gin;
    const float* kg = pvar(c, rs + "rnn/gru_cell/gates/kernel");
    const float* kcn = pvar(c, rs + "rnn/gru_cell/candidate/kernel");
    float* WghT = WT;                       // [2RD][RD]
    float* WchT = WT + 2L * RD * RD;        // [RD][RD]
    const bool gseq = c->sw.fe_gru_seq && fe_gru_seq_ok(B, RD);
    if (gseq) {  // the whole reverse recurrence in one work-group (fp32 MFMA)
      fe_gru_bwd_seq(kg + (long)gin * 2 * RD, kcn + (long)gin * RD, c->fGR[r].as<float>(), c->fGU[r].as<float>(),
                     c->fGCC[r].as<float>(), c->fHG[r].as<float>(), B, T2, RD, c->fDH.as<float>(), c->fDCP.as<float>(),
                     c->fDGP.as<float>(), s, tr_prec(c) == 2);
    } else {
      tr_transpose(kg + (long)gin * 2 * RD, RD, 2 * RD, 2 * RD, WghT, RD, s);
      tr_transpose(kcn + (long)gin * RD, RD, RD, RD, WchT, RD, s);
    }
    for (int t = gseq ? -1 : T2 - 1; t >= 0; --t) {
      fe_gru_bwd_a(c->fDH.as<float>(), c->fGU[r].as<float>(), c->fGCC[r].as<float>(), c->fHG[r].as<float>(), B, RD, t,
                   c->fDCP.as<float>(), c->fDHA.as<float>(), s);
      tr_gemm(c, B, RD, RD, c->fDCP.as<float>() + (long)t * B * RD, RD, WchT, RD, c->fDRH.as<float>(), RD, s);
      fe_gru_bwd_b(c->fDRH.as<float>(), c->fGR[r].as<float>(), c->fGU[r].as<float>(), c->fHG[r].as<float>(),
                   c->fGCC[r].as<float>(), c->fDH.as<float>(), B, RD, t, c->fDGP.as<float>(), c->fDHA.as<float>(), s);
      tr_gemm(c, B, RD, 2 * RD, c->fDGP.as<float>() + (long)t * B * 2 * RD, 2 * RD, WghT, RD, c->fDH.as<float>(), RD, s,
              nullptr, c->fDHA.as<float>(), RD);
    }
    // recurrent weight gradients over all steps: d Wg_h = Σ h(t)ᵀ dGP(t), d Wc_h = Σ (r h)(t)ᵀ dCP(t)
    const long R2 = (long)T2 * B;
    tr_transpose(c->fHG[r].as<float>(), R2, RD, RD, FB, R2, s);
    tr_gemm(c, RD, 2 * RD, (int)R2, FB, R2, c->fDGP.as<float>(), 2 * RD, gvar(c, rs + "rnn/gru_cell/gates/kernel") +
            (long)gin * 2 * RD, 2 * RD, s);
    tr_transpose(c->fGRH[r].as<float>(), R2, RD, RD, FB, R2, s);
    tr_gemm(c, RD, RD, (int)R2, FB, R2, c->fDCP.as<float>(), RD, gvar(c, rs + "rnn/gru_cell/candidate/kernel") +
            (long)gin * RD, RD, s);
    // input side over all (n, t) rows: DXG = [dGP | dCP] in (n, t) order
    fe_gru_dxg(c->fDGP.as<float>(), c->fDCP.as<float>(), B, T2, RD, c->fDXG.as<float>(), s);
    const float* x6 = c->f_adain ? c->fADX.as<float>() : c->fRY[r][5].as<float>();
    tr_transpose(x6, R2, gin, gin, FB, R2, s);
    tr_gemm(c, gin, 2 * RD, (int)R2, FB, R2, c->fDXG.as<float>(), 3 * RD, gvar(c, rs + "rnn/gru_cell/gates/kernel"),
            2 * RD, s);
    tr_gemm(c, gin, RD, (int)R2, FB, R2, c->fDXG.as<float>() + 2 * RD, 3 * RD,
            gvar(c, rs + "rnn/gru_cell/candidate/kernel"), RD, s);
    tr_colsum(c, c->fDXG.as<float>(), R2, 2 * RD, 3 * RD, gvar(c, rs + "rnn/gru_cell/gates/bias"), s);
    tr_colsum(c, c->fDXG.as<float>() + 2 * RD, R2, RD, 3 * RD, gvar(c, rs + "rnn/gru_cell/candidate/bias"), s);
    float* dY = c->fDY.as<float>();
    tr_transpose(kg, gin, 2 * RD, 2 * RD, WT, gin, s);  // [2RD][gin]
    tr_gemm(c, (int)R2, gin, 2 * RD, c->fDXG.as<float>(), 3 * RD, WT, gin, dY, gin, s);
    tr_transpose(kcn, gin, RD, RD, WT, gin, s);
    tr_gemm(c, (int)R2, gin, RD, c->fDXG.as<float>() + 2 * RD, 3 * RD, WT, gin, dY, gin, s, nullptr, dY, gin);
    if (!c->f_adain) {
      conv_bwd(r, dY);
      continue;
    }
    // AdaIN: the restyle's backward splits d map into the speaker map's gradient (in place) and the
    // emotion map's (through its moments), then both stacks run backward
    const int C6 = f.reference_filters[5], HW = T2 * (gin / C6);
    fe_ad_mix_bwd(dY, c->fRY[1][5].as<float>(), c->fRY[0][5].as<float>(), B, HW, C6, c->fADM.as<float>() + (long)B * C6 * 2,
                  c->fADM.as<float>(), c->fADS.as<float>(), dY, c->fDYE.as<float>(), s);
    conv_bwd(1, dY);  // (din is read by the top layer's ReLU mask before any col2im writes dY)
    conv_bwd(0, c->fDYE.as<float>());
  }
  // BiLSTM BPTT (the decoder's DMEM rows carry d enc_out in columns [0, 2U))
  for (int d = 0; d < 2; ++d) {
    const float* k = pvar(c, fe_lstm_scope(d) + "kernel");
    tr_transpose(k + (long)C * 4 * U, U, 4 * U, 4 * U, c->fLWhT.as<float>() + (long)d * 4 * U * U, U, s);
    tr_transpose(k, C, 4 * U, 4 * U, c->fLWxT.as<float>() + (long)d * 4 * U * C, C, s);
  }
  TT2_HIP(hipMemsetAsync(c->fDHC.p, 0, c->fDHC.bytes, s));
  TT2_HIP(hipMemsetAsync(c->fDCC.p, 0, c->fDCC.bytes, s));
  FeLstm l{};
  l.GA = c->fGA.as<float>(); l.CN = c->fCN.as<float>(); l.CS = c->fCS.as<float>(); l.HS = c->fHS.as<float>();
  l.zm = enczm; l.lens = lens; l.B = B; l.T = T; l.U = U; l.zo = f.zoneout;
  l.DENC = c->DMEM.as<float>(); l.ld_denc = D; l.DZ = c->fDZ.as<float>(); l.DHC = c->fDHC.as<float>();
  l.DCC = c->fDCC.as<float>(); l.DHP = c->fDHP.as<float>();
  if (fe_enc_fused(c)) {  // d h carried = dZ(t+1)·Wh^T + its direct part, fused with the cell backward
    const long Bp = (B + 31) & ~31L;
    for (int d = 0; d < 2; ++d)
      tr_tf_weights_f32(pvar(c, fe_lstm_scope(d) + "kernel") + (long)C * 4 * U, (long)4 * U, 0, U, 4 * U, U / 32,
                        (int)TF_PLAIN, U, c->fTWb.as<__bf16>() + (long)d * 4 * U * U, s);
    TT2_HIP(hipMemsetAsync(c->fDZh.p, 0, c->fDZh.bytes, s));  // dZ(T) = 0
    TT2_HIP(hipMemsetAsync(c->fDHP.p, 0, c->fDHP.bytes, s));
    TrFused e{};
    e.Wt = c->fTWb.as<__bf16>(); e.wdir = (long)4 * U * U; e.K = 4 * U; e.B = B; e.H = U; e.T = T; e.lens = lens;
    e.zm = enczm; e.zo = f.zoneout; e.GA = c->fGA.as<float>(); e.CN = c->fCN.as<float>(); e.CS = c->fCS.as<float>();
    e.DENC = c->DMEM.as<float>(); e.ld_denc = D; e.DZ = c->fDZ.as<float>(); e.DCC = c->fDCC.as<float>();
    e.DHP = c->fDHP.as<float>(); e.DZh = c->fDZh.as<__bf16>(); e.adir = 2 * Bp * 4 * U;
    for (int t = T - 1; t >= 0; --t) {
      e.t = t;
      tr_fused_enc_step(e, true, s);
    }
  } else {
    for (int t = T - 1; t >= 0; --t) {
      l.t = t;
      fe_lstm_cell_bwd(l, s);
      for (int d = 0; d < 2; ++d)
        tr_gemm(c, B, U, 4 * U, c->fDZ.as<float>() + ((long)d * T + t) * B * 4 * U, 4 * U,
                c->fLWhT.as<float>() + (long)d * 4 * U * U, U, c->fDHC.as<float>() + (long)d * B * U, U, s, nullptr,
                c->fDHP.as<float>() + (long)d * B * U, U);
    }
  }
  for (int d = 0; d < 2; ++d) {  // recurrent weights: Σ_t HS(t)ᵀ DZ(t); biases
    const long R = (long)T * B;
    tr_transpose(c->fHS.as<float>() + (long)d * (T + 1) * B * U, R, U, U, FB, R, s);
    tr_gemm(c, U, 4 * U, (int)R, FB, R, c->fDZ.as<float>() + (long)d * T * B * 4 * U, 4 * U,
            gvar(c, fe_lstm_scope(d) + "kernel") + (long)C * 4 * U, 4 * U, s);
    tr_colsum(c, c->fDZ.as<float>() + (long)d * T * B * 4 * U, R, 4 * U, 4 * U, gvar(c, fe_lstm_scope(d) + "bias"), s);
  }
  fe_lstm_dxp(c->fDZ.as<float>(), lens, B, T, U, c->fdXP.as<float>(), s);
  const float* X3 = c->fEY[f.enc_conv_layers].as<float>();
  tr_transpose(X3, M, C, C, FB, M, s);
  float* dxn = c->fdA.as<float>();
  float* dxo = c->fdB.as<float>();
  for (int d = 0; d < 2; ++d) {
    tr_gemm(c, C, 4 * U, (int)M, FB, M, c->fdXP.as<float>() + d * 4 * U, 8 * U, gvar(c, fe_lstm_scope(d) + "kernel"),
            4 * U, s);
    tr_gemm(c, (int)M, C, 4 * U, c->fdXP.as<float>() + d * 4 * U, 8 * U, c->fLWxT.as<float>() + (long)d * 4 * U * C, C,
            dxn, C, s, nullptr, d ? dxn : nullptr, C);
  }
  // encoder convolutions backward (dropout -> BN -> ReLU -> conv)
  for (int i = f.enc_conv_layers - 1; i >= 0; --i) {
    const std::string sc = fe_conv_scope(i + 1);
    const float* mean = BN + (long)i * 2 * 512;
    const float* var = mean + 512;
    float* dz = c->fDZc.as<float>();
    const bool bplanes = c->fePl.p && tr_prec(c) == 2;
    __bf16* bpl = reinterpret_cast<__bf16*>(c->fePl.p);
    fe_bn_bwd(c, dxn, encm ? encm + (long)i * M * C : nullptr, c->fEA[i].as<float>(), M, C, mean, var, sc, 2,
              c->fDY.as<float>(), dz, s, bplanes ? bpl : nullptr, T);
    tr_colsum(c, dz, M, C, C, gvar(c, sc + "conv1d/bias"), s);
    const int cin = i == 0 ? E : C, pad = (K - 1) / 2;
    const float* xin = i == 0 ? c->fEX.as<float>() : c->fEY[i].as<float>();
    if (c->sw.blas && tr_prec(c) == 2 && 2.0 * K * cin * (double)C * M >= kTrBigMinFlops) {
      KcConvA cv;  // im2colᵀ gathered straight into gemm_bf16_kc's bf16 operand copy
      cv.x = xin; cv.xs_b = (long)T * cin; cv.xs_t = cin; cv.B = B; cv.T = T; cv.C = cin; cv.kw = K; cv.pad = pad;
      gemm_bf16_kc(K * cin, C, (int)M, nullptr, 0, dz, C, gvar(c, sc + "conv1d/kernel"), C, c->blasA, c->blasB,
                   c->blasP, s, false, &cv);
      ++c->blas_calls;
    } else {
      tr_im2col_t(xin, (long)T * cin, (long)cin, B, T, cin, K, pad, FB, M, s);
      tr_gemm(c, K * cin, C, (int)M, FB, M, dz, C, gvar(c, sc + "conv1d/kernel"), C, s);
    }
    tr_conv_flip(pvar(c, sc + "conv1d/kernel"), K, cin, C, WT, s);
    if (bplanes) {  // input gradient: conv of the dz planes with the flipped kernel
      __bf16* bwt = reinterpret_cast<__bf16*>(c->feWt.p);
      kc_transpose_bf16(WT, K * C, cin, cin, bwt, K * C, (cin + 255) / 256 * 256, s);
      conv_bf16_planes(bpl, C, B, T, K, bwt, (long)K * C, cin, nullptr, ACT_NONE, dxo, cin, s);
    } else {
      GemmArgs g;
      g.a_mode = A_CONV1D; g.M = (int)M; g.N = cin; g.T = T; g.kw = K; g.pad = K - 1 - pad;
      g.A = dz; g.C = C; g.xs_b = (long)T * C; g.xs_t = C; g.K = K * C;
      g.Bw = WT; g.ldb = cin; g.Cout = dxo; g.ldc = cin;
      tr_gemm_run(c, g, s);
    }
    std::swap(dxn, dxo);
  }
  fe_embed_bwd(ids, dxn, M, E, f.n_symbols, gvar(c, vn("inputs_embedding")), s, FB,
               (long)(c->fFBUF.bytes / sizeof(float)));  // FB is free after the conv loop
}

}  // namespace tt2
