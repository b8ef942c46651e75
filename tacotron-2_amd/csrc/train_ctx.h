// Internal header of the training step: the context, its environment switches, the variable-name
// helpers and the host helpers that train.hip (decoder, Postnet, C ABI) and train_front_host.hip
// (encoder, reference encoders, GST, style losses) share.  Everything a helper needs comes in through
// the context it is handed: there is no per-thread or per-process state.
#pragma once
#include <functional>
#include <initializer_list>
#include <utility>

#include "common.h"
#include "gemm.h"

namespace tt2 {

struct TrVar {
  std::string name;
  std::vector<int64_t> shape;
  long off = 0, n = 0;
  bool reg = false;
};

// Environment switches of the training library, read ONCE in tt2_train_create (tr_read_switches) and
// kept with the context: two contexts built under different environments keep their own values, and
// a change after create has no effect on a live context.  Parsed by env_on / env_int (common.h).
// The one exception is the test hook TT2_TP_FORCE_FAIL, read at every persistent forward launch
// (tr_persist_forward) so a test can fail one step of a live trainer.
struct TrSwitches {
  bool blas = true;         // TT2_TRAIN_BLAS=0: the large plain products on gemm_x3_kernel too (no gemm_bf16_kc)
  bool values16 = true;     // TT2_TR_VALUES16=0: no bf16 copy of the values for the context / d align reads
  bool fe_direct = true;    // TT2_FE_CONV_DIRECT=0: the refnet conv2d backward as im2col + GEMM + col2im
  bool fe_gru_seq = true;   // TT2_FE_GRU_SEQ=0: the refnet GRU as per-step launches (4 per step)
  bool persist = true;      // TT2_TR_PERSIST=0: the decoder forward as per-step launches
  bool persist_bwd = true;  // TT2_TR_PERSIST_BWD=0: the decoder backward as per-step launches
  bool pn_planes = true;    // TT2_PN_PLANES=0: Postnet / encoder convs on the implicit-im2col gemm_x3_kernel
  bool fused = true;        // TT2_TR_FUSED=0: split-K products + cell launches instead of k_tr_fused
  bool e2 = true;           // TT2_TR_E2=0: the 1024-thread attention energy kernels
  bool attq = true;         // TT2_TR_ATTQ=0: the attention backward as two per-tile launches
  bool dwloc_cum = true;    // TT2_TR_DWLOC_CUM=0: d W_loc from the stored location features (FALL + k_tr_dwloc)
  bool tb_dgt = true;       // TT2_TB_DGT=0: the persistent backward does not stage bf16(dG)^T for the weight gradients
  int tp_oc = 1;            // TT2_TP_OC: placement of the persistent forward's off-chain products (0 / 1)
  // TT2_{TP,TB,ATTQ}_STAMP=<step>: stage stamps of that step of the persistent forward / persistent
  // backward / k_tr_att_bwd_q, written as raw int64 to TT2_*_STAMP_FILE (diagnostic; < 0: off)
  int tp_stamp = -1, tb_stamp = -1, attq_stamp = -1;
  std::string tp_stamp_file, tb_stamp_file, attq_stamp_file;  // tp_stamps.bin, tb_stamps.bin, attq_stamps.bin
};

}  // namespace tt2

using namespace tt2;  // (the C ABI's opaque context type lives at global scope)

struct tt2_train_ctx {
  int dev = 0;
  TrSwitches sw;  // environment switches as tt2_train_create found them
  hipStream_t stream = nullptr;
  tt2_train_config cfg{};
  int B = 0, Tm = 0, Tin = 0, D = 0, NM = 0, P = 0, H = 0, A = 0, F = 0, KW = 0;
  int LX1 = 0;  // P + D + H
  int R = 1;    // outputs_per_step: frames per decoder step
  std::vector<TrVar> vars;
  std::map<std::string, int> index;
  long total = 0;
  WeightMap host;
  bool finalized = false;
  long step_count = 0;
  // flat parameter / gradient / Adam buffers
  DevBuf params, grads_own, adam_m, adam_v;
  float* grads = nullptr;  // grads_own or a caller-bound buffer
  // transposed weights (refreshed every step)
  DevBuf K1T, K2T, WqT, WfT, WsT, WmT, Wp2T;
  // activations
  DevBuf values, keys, X1, X2, PIN, G1, G2, C1, C2, CN1, CN2, Q, ALIGN, CUM, P1, XIN, FR, ST;
  // backward
  DevBuf dFR, dST, dPIN, dX1, dX2, dG1, dG2, DC1, DC2, R1, R2, DQ, DCTX, DKEYS, DCUM;
  DevBuf dV, dBA, dKC, dBC, DVAL, DMEM, dZ, dPre, TBUF, part, red, kpart;
  DevBuf DF2, DCUM2, PQ2, SC2;
  DevBuf DWGP;  // [B][NT][32][A] k_tr_att_bwd_q's d W_loc accumulators (TrAtt::DWGP)
  DevBuf SS;   // [T][B] smoothing: Σ sigmoid(e) per step (TrAtt::SS)
  DevBuf DWG;  // [32][A] k_tr_dwloc_cum: Σ cum_{t-1}·du per tap (+ the Σ du row)  // k_tr_att_bwd_q: df / d cum / d query / Σ a·d cum partials by step parity
  DevBuf TH, E, DF, PQ, FALL, ALN;
  // the large plain products (tr_gemm_big)
  DevBuf blasA, blasB, blasP;  // gemm_bf16_kc: bf16 operand copies, split-K partials
  long blas_calls = 0;
  // bf16 copies of the recurrent weights in both layouts (precision = bf16), refreshed per step
  DevBuf hK1, hK1T, hK2, hK2T, hWq, hWqT;
  DevBuf X1h, X2h;  // bf16 shadows of the X1 / X2 rows (inputs of the fused LSTM products)
  DevBuf dGh;       // bf16 shadows of one step's dG2 | dG1 rows (fused backward products)
  DevBuf tK1T, tK2T, tWq, tK2, tK1;  // the fused products' weights in TF layout (k_tr_tf_weights)
  // Postnet training (cfg.postnet): PA[i] activations (pre-BN), PX[i] layer inputs (PX[0] unused:
  // layer 1 reads the clipped frames), batch stats, projection, scratch
  DevBuf PA[8], PX[9];  // postnet_layers <= 8
  DevBuf BNM, BNV, PPRJ, dPP, DYb, DZb, dPXa, dPXb, WFLIP, PWT, CLIPM, pn_part;
  int PL = 0, PC = 0, PK = 0;
  bool pn_masks = false;
  int T_last = 0, Tin_last = 0;  // decoder steps / encoder positions of the last forward_backward
  int Tf_last = 0;               // its frame count T_last * R
  DevBuf FRT;                    // R > 1: the clipped frames time-major [T_f][B][NM] (the Postnet's input)
  bool pn_ran = false;  // batch stats of the last forward are valid (moving averages in apply)
  // bf16 Postnet convolutions over padded planes (gemm.h conv_bf16_planes): the layer input / dz
  // planes (pad rows zeroed when the shape changes) and the transposed bf16 weights of one layer
  DevBuf pnPl, pnWt;
  DevBuf fePl, feWt;  // the same for the text encoder's convolutions (TT2_PN_PLANES gates both)
  int fe_pl_B = -1, fe_pl_T = -1;
  DevBuf values16;         // bf16 values for the per-step context / d align reads (TT2_TR_VALUES16)
  int pn_pl_B = -1, pn_pl_T = -1;
  bool pn_planes = false;
  hipStream_t last_stream = nullptr;  // stream of the last forward_backward / apply (read-backs)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_ms = 0.f;
  // front end (cfg.frontend: encoder + reference encoders + GST, train_front.hip)
  int f_nref = 0, f_gin = 0, f_T2 = 0, f_T2max = 0;
  bool f_ran = false;
  // cfg.adain (ReferenceEncoderAdaIn, modules.py:66-107): stacks r = 0 (emotion mel) and r = 1 (speaker
  // mel) without batch norm, the speaker map restyled by the emotion map's moments, one GRU + dense
  // (r = 1 buffers): fADX the restyled map (GRU input), fADM moments [2 (emt, spk)][B][C][2], fADS the
  // backward's per-channel sums, fDYE the emotion stack's map gradient
  bool f_adain = false;
  DevBuf fADX, fADM, fADS, fDYE;
  DevBuf fTWf, fTWb, fHSh, fDZh;  // encoder BiLSTM fused steps: TF-layout weights and state / dZ shadows
  DevBuf fEX, fEA[8], fEY[9], fXP, fGZ, fGA, fCN, fCS, fHS, fENC, fMEM, fSTY, fDSTY, fDZ, fDHC, fDCC, fDHP, fdXP, fdA,
      fdB, fLWxT, fLWhT;
  DevBuf fRA[2][6], fRY[2][6], fXG[2], fGR[2], fGU[2], fGCC[2], fGRH[2], fHG[2], fREF[2], fGG, fGC, fFBUF, fDY, fDY2,
      fDZc;
  DevBuf fGq, fGkk, fGv, fGnv, fGbb, fGsum, fdREF, fDZD, fDH, fDHA, fDRH, fDCP, fDGP, fDXG, fWT, fBN, fpart;
  // loss masks (cfg.mask_decoder): target lengths [B] on the device, their sum
  DevBuf TLEN;
  bool has_tlen = false;
  // style-embedding losses (cfg.n_emt / n_spk / orthog_weight): labels [2][B], the extra d refnet
  // outputs [2][B][128], classifier logit gradients [B][max(n)], the orthogonality product [B][B]
  DevBuf sLAB, sXREF, sDL, sOM;
  bool has_labels = false;
  long tlen_sum = 0;
  int tlen_max = 0;
  // teacher-forcing draw (tt2_train_set_teacher_forcing): feed[t] = 1 target frame t-1, 0 own frame
  std::vector<uint8_t> feed;
  // free-running steps: prenet-1 kernel transposed [P][NM], per-step scratch
  DevBuf W1T, sDZ, sDP, sDX;
  // persistent forward (train_persist.hip; tp_on = sw.persist on a device that fits): exchange
  // buffers, energy granules, flags + control words, the prenet rows in bf16 fragment layout
  DevBuf tpCX, tpH1X, tpZ1X, tpH2X, tpZ2X, tpEX, tpCtl, tpPre, tpStamps, tpKWT;
  bool tp_on = false, tp_last = false, tp_check = false;
  // persistent backward (train_bwd_persist.hip): exchange buffers, flags + control words
  DevBuf tbG1X, tbG2X, tbP1X, tbP2X, tbQX, tbCtl, tbW1F, tbPK, tbDGT1, tbDGT2, tbDGR1;
  DevBuf reg_segs;  // [nreg] (offset, size) of the regularised variables (tr_regularize)
  int nreg = 0;
  bool tb_dgt = false;  // the last persistent backward wrote bf16(dG)^T for the weight-gradient GEMMs
  bool tb_dgr = false;  // ... and bf16(dG1) row-major for the d X1 product
  bool tb_on = false, tb_last = false, tb_check = false;
  int* tb_ctl_dev = nullptr;
  int* tp_ctl_dev = nullptr;  // control words of the last persistent forward (device)
  int* tp_ctl_host = nullptr;  // pinned [2]: the launch's control words, checked at the next read-back
};

namespace tt2 {

inline int tr_prec(const tt2_train_ctx* c) { return c->cfg.precision ? 2 : 0; }  // GemmArgs::split16 (0 fp32, 2 bf16)

// ---- variable names ------------------------------------------------------------------------------
inline std::string vn(const char* s) { return std::string("Tacotron_model/inference/") + s; }
inline float* pvar(tt2_train_ctx* c, const std::string& n) { return c->params.as<float>() + c->vars[c->index.at(n)].off; }
inline float* gvar(tt2_train_ctx* c, const std::string& n) { return c->grads + c->vars[c->index.at(n)].off; }
inline std::string fe_conv_scope(int i) {
  return vn("encoder_convolutions/conv_layer_") + std::to_string(i) + "_encoder_convolutions/";
}
inline std::string fe_ref_scope(const tt2_train_ctx* c, int r) {
  return vn(c->f_adain ? "refnet/" : r == 0 ? "refnet_emt/" : "refnet_spk/");
}

// ---- host helpers defined in train.hip -------------------------------------------------------------
inline unsigned nblk(long n, int t = 256) { return (unsigned)((n + t - 1) / t); }
void tr_transpose(const float* src, long rows, long cols, long lds, float* dst, long ldd, hipStream_t s);
void tr_colsum(tt2_train_ctx* c, const float* in, long M, int N, long ld, float* out, hipStream_t s);
void tr_zero_many(std::initializer_list<std::pair<void*, size_t>> l, hipStream_t s);
void tr_redzones(tt2_train_ctx* c, const char* phase);
// products in the context's precision, split-K scratch and (bf16, large) gemm_bf16_kc operand copies
constexpr double kTrBigMinFlops = 2.0e10;
bool tr_gemm_big(tt2_train_ctx* c, int M, int N, int K, const float* A, long lda, const float* Bw, long ldb, float* C,
                 long ldc, hipStream_t s);
void tr_gemm(tt2_train_ctx* c, int M, int N, int K, const float* A, long lda, const float* Bw, long ldb, float* C,
             long ldc, hipStream_t s, const float* bias = nullptr, const float* residual = nullptr, long ldr = 0,
             int act = ACT_NONE, const DevBuf* bt16 = nullptr, long ldbt = 0);
void tr_gemm_xtg(tt2_train_ctx* c, int M, int N, int K, const float* X, long ldx, const float* dG, long ldg, float* C,
                 long ldc, float* TBUF, hipStream_t s, const __bf16* dgt = nullptr);
int tr_gemm_raw(tt2_train_ctx* c, int M, int N, int K, const float* A, long lda, const float* Bw, long ldb,
                hipStream_t s, const DevBuf* bt16 = nullptr, long ldbt = 0);
void tr_gemm_run(tt2_train_ctx* c, GemmArgs& g, hipStream_t s);

// ---- launchers of train.hip kernels the front end shares with the decoder / Postnet -------------------
// training-mode batch norm over the M rows of [M][C] (described at their definitions)
void tr_bn_stats(const float* x, long M, int C, long cap, float* part, float* mean, float* var, hipStream_t s);
void tr_bn_fwd(const float* a, long M, int C, const float* mean, const float* var, const float* gamma,
               const float* beta, float eps, const uint8_t* keep, float* y, __bf16* planes, int T, hipStream_t s);
void tr_bn_bwd(const float* dxn, const uint8_t* keep, const float* a, long M, int C, const float* mean,
               const float* var, float eps, const float* gamma, float* dgamma, float* dbeta, long cap, float* part,
               float* sums, int act, float* dy, float* dz, __bf16* planes, int T, hipStream_t s);
void tr_im2col_t(const float* x, long xs_b, long xs_t, int B, int T, int C, int kw, int pad, float* out, long M,
                 hipStream_t s);
void tr_conv_flip(const float* w, int kw, int cin, int cout, float* wf, hipStream_t s);
void tr_rows_copy(const float* src, long lds, long rows, int cols, float* dst, long ldd, const float* add, long lda,
                  hipStream_t s);
void tr_sum_final(const float* part, int nb, float scale, float* out, int mode, hipStream_t s);
void tr_tf_weights_f32(const float* src, long ld, int transposed, int N, int K, int ncg, int mode, int H, __bf16* dst,
                       hipStream_t s);

// the padded bf16 input planes of conv_bf16_planes (gemm.h CX_* layout): element i of rows b·T + t
__device__ __forceinline__ void pn_plane_put(__bf16* planes, int T, long i, int C, float v) {
  const long m = i / C;
  const int c = (int)(i - m * C), b = (int)(m / T), t = (int)(m - (long)b * T);
  planes[(CX_G + (long)b * (T + 2 * CX_P) + CX_P + t) * C + c] = (__bf16)v;
}

// k_tr_fused (train.hip): product + consumer epilogue of one recurrent step in one launch
enum { TF_FWD = 0, TF_BWD_H = 1, TF_BWD_S = 2, TF_PLAIN = 3, TF_EFWD = 4, TF_EBWD = 5 };
constexpr int TLG_U = 8, TLG_NT = 512, TLG_KSMAX = 16;
struct TrFused {
  const __bf16* Ah;  // this step's bf16 input rows, TF layout of width K, or
  const float* Af;   // fp32 input rows (TF_BWD_H)
  long lda;
  int af_parts;      // > 1: each Af row is the sum of af_parts partial rows af_pstride apart (in order)
  int af_pstride;
  const __bf16* Wt;  // W^T in TF layout, column-group order (k_tr_tf_weights)
  int K, B, H, N;
  int t, layer;
  float z;
  const uint8_t* zm;     // [T][4][B][H] zoneout keep masks or null
  const float* G;        // fwd: out [B][4H] activated gates; bwd: in
  const float* bias;     // fwd
  const float* c_prev;   // [B,H]
  const float* hz_prev;  // fwd, strided
  long ld_hz_prev;
  float* cn;             // fwd out / bwd in [B,H]
  float* c_out;          // fwd [B,H]
  float* h_out;          // fwd strided h_new
  long ld_h;
  float* hz_out;         // fwd strided zoned h
  long ld_hz;
  __bf16* h_out_h;       // fwd bf16 TF-layout shadows (step block base, width ld_*_h, column offset
  long ld_h_h;           // *_col0) or null
  __bf16* hz_out_h;
  long ld_hz_h;
  int h_col0, hz_col0;
  const float* dh_ext;   // bwd: d h_new from the frame projection (strided) or null
  long ld_dh;
  float* side;           // TF_BWD_S: d hz2_{t-1} out (strided), = product + side_res[.][H + n]
  long ld_side;
  const float* side_res;
  long ld_side_res;
  const float* dhz;      // bwd: d(zoned h_t) from step t+1 (strided)
  long ld_dhz;
  float* DC;             // bwd [B,H] in/out
  float* dG;             // bwd out [B][4H]
  __bf16* dGh;           // bwd bf16 shadow of dG or null
  float* R;              // bwd [B][ldr] at off_r + n
  long ldr;
  int off_r;
  float* C;              // TF_PLAIN out (ld ldc) = product + residual
  long ldc;
  const float* residual;
  long ldres;
  // encoder BiLSTM (TF_EFWD / TF_EBWD, FeLstm's buffers; H = U, both directions in one launch)
  const int* lens;
  int T;                 // encoder steps
  float zo;
  long wdir, adir;       // per-direction strides of Wt and of the bf16 state shadow (elements)
  const float* XP;       // [B][T][8U] input projections (+ bias)
  float* GA; float* CN; float* CS; float* HS; float* ENC;
  __bf16* HSh;           // [2][T+1][Bp][U] TF layout: h state shadow (EFWD: A operand and output)
  const float* DENC; long ld_denc;
  float* DZ; float* DCC; float* DHP;
  __bf16* DZh;           // [2 dirs][2 slots][Bp][4U] TF layout: dZ shadow (EBWD: A of step t-1)
};
// one encoder BiLSTM step (both directions) of k_tr_fused: TF_EFWD, or TF_EBWD when backward
void tr_fused_enc_step(const TrFused& e, bool backward, hipStream_t s);

// ---- front end (train_front_host.hip) ----------------------------------------------------------------
void tr_front_build_vars(tt2_train_ctx* c,
                         const std::function<void(const std::string&, std::vector<int64_t>, bool)>& add);
void tr_front_alloc(tt2_train_ctx* c);
void tr_front_forward(tt2_train_ctx* c, const int* ids, const int* lens, const float* const* refs, int T_ref,
                      const uint8_t* encm, const uint8_t* enczm, int T, hipStream_t s);
void tr_front_backward(tt2_train_ctx* c, const int* ids, const int* lens, const float* const* refs, int T_ref,
                       const uint8_t* encm, const uint8_t* enczm, int T, hipStream_t s);
bool tr_style_on(const tt2_train_ctx* c);

}  // namespace tt2
