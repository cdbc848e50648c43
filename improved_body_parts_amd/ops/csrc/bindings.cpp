// Python bindings for the CDNA4 kernel library.
#include <torch/extension.h>

using torch::Tensor;

// bn_act.hip
std::vector<int64_t> bn_v8_geometry(int64_t M, int64_t C);
std::vector<Tensor> bn_stats(const Tensor& x_mc, int64_t C);
std::vector<Tensor> bn_finalize(
    const Tensor& sums, const Tensor& sumsq, int64_t M, const Tensor& gamma,
    const Tensor& beta, const c10::optional<Tensor>& running_mean,
    const c10::optional<Tensor>& running_var,
    const c10::optional<Tensor>& num_batches, double momentum, double eps);
std::vector<Tensor> bn_stats_finalize(
    const Tensor& x_mc, int64_t C, const Tensor& gamma, const Tensor& beta,
    const c10::optional<Tensor>& running_mean,
    const c10::optional<Tensor>& running_var,
    const c10::optional<Tensor>& num_batches, double momentum, double eps);
Tensor bn_act_fwd(const Tensor& x, const Tensor& scale, const Tensor& shift,
                  const c10::optional<Tensor>& residual, double slope, bool act);
std::vector<Tensor> bn_act_bwd(const Tensor& dy, const Tensor& y, const Tensor& x,
                               const c10::optional<Tensor>& mean,
                               const c10::optional<Tensor>& invstd,
                               double slope, bool act, bool need_xhat, int64_t C);
Tensor bn_act_bwd_apply(const Tensor& dpre, const Tensor& x, const Tensor& mean,
                        const Tensor& invstd, const Tensor& gamma,
                        const c10::optional<Tensor>& sum_dpre,
                        const c10::optional<Tensor>& sum_dxhat, int64_t C);

// spatial.hip
std::vector<Tensor> maxpool2x2_fwd(const Tensor& x, int64_t N, int64_t H,
                                   int64_t W, int64_t C);
Tensor maxpool2x2_bwd(const Tensor& dy, const Tensor& arg, int64_t N, int64_t H,
                      int64_t W, int64_t C);
Tensor upsample2x_fwd(const Tensor& x, int64_t N, int64_t H, int64_t W, int64_t C);
Tensor upsample2x_bwd(const Tensor& dy, int64_t N, int64_t H, int64_t W, int64_t C);
Tensor se_reduce(const Tensor& a, const c10::optional<Tensor>& b, int64_t N,
                 int64_t HW, int64_t C);
Tensor se_scale(const Tensor& x, const Tensor& s, const c10::optional<Tensor>& addc,
                int64_t N, int64_t HW, int64_t C);
Tensor se_gate(const Tensor& pooled, const Tensor& w1, const Tensor& b1,
               const Tensor& w2, const Tensor& b2, double slope,
               double pool_scale);
std::vector<Tensor> se_layer_grouped(const std::vector<Tensor>& xs,
                                     const std::vector<Tensor>& w1s,
                                     const std::vector<Tensor>& b1s,
                                     const std::vector<Tensor>& w2s,
                                     const std::vector<Tensor>& b2s,
                                     double slope);

// loss.hip
Tensor focal_l2_fwd(const Tensor& pred, const Tensor& gt, const Tensor& mask,
                    int64_t heat_start, int64_t bkg_start, int64_t gamma,
                    double mtw, double ktw, double alpha, double beta);
Tensor focal_l2_bwd(const Tensor& pred, const Tensor& gt, const Tensor& mask,
                    const Tensor& stack_gscale, int64_t heat_start,
                    int64_t bkg_start, int64_t gamma, double mtw, double ktw,
                    double alpha, double beta);

// conv_mfma.hip
// geom = N H W Cin Cout KH KW stride pad_h pad_w dil_h dil_w Ho Wo zs
Tensor conv_mfma_fwd(const Tensor& x, const Tensor& w_packed,
                     const std::vector<int64_t>& geom,
                     const c10::optional<Tensor>& scale,
                     const c10::optional<Tensor>& shift,
                     const c10::optional<Tensor>& residual, bool act,
                     const c10::optional<Tensor>& residual_post,
                     const c10::optional<Tensor>& residual_post2,
                     const c10::optional<Tensor>& x2);

std::vector<Tensor> conv_mfma_fwd_grouped(
    const std::vector<Tensor>& xs, const std::vector<Tensor>& ws_packed,
    const std::vector<std::vector<int64_t>>& geom,
    const std::vector<c10::optional<Tensor>>& scales,
    const std::vector<c10::optional<Tensor>>& shifts,
    const std::vector<c10::optional<Tensor>>& residuals,
    const std::vector<bool>& acts,
    const std::vector<c10::optional<Tensor>>& residual_posts,
    const std::vector<c10::optional<Tensor>>& residual_post2s);

std::vector<int64_t> conv_mfma_tile_plan(int64_t M, int64_t Cout, int64_t K);
std::vector<int64_t> conv_mfma_conv_plan(const Tensor& x,
                                         const Tensor& w_packed,
                                         const std::vector<int64_t>& geom);

void pack_conv_weight(const Tensor& w, Tensor& fwd_pack,
                      const c10::optional<Tensor>& dgrad_pack);

void pack_upfold_weight(const Tensor& w, Tensor& out);
void pack_cat_weight(const Tensor& wa, const Tensor& wb,
                     const c10::optional<Tensor>& scale_a,
                     const c10::optional<Tensor>& scale_b,
                     const c10::optional<Tensor>& shift_a,
                     const c10::optional<Tensor>& shift_b, Tensor& out,
                     Tensor& shift_out);
Tensor conv_mfma_upfold_fwd(const Tensor& x_low, const Tensor& packs,
                            const std::vector<int64_t>& geom,
                            const c10::optional<Tensor>& scale,
                            const c10::optional<Tensor>& shift, bool act,
                            const c10::optional<Tensor>& residual_post,
                            const c10::optional<Tensor>& residual_post2);
std::vector<int64_t> conv_mfma_upfold_plan(int64_t M_low, int64_t Cout,
                                           int64_t Cin);

// conv_wgrad.hip
Tensor conv_mfma_wgrad(const Tensor& x, const Tensor& dy, int64_t N, int64_t H,
                       int64_t W, int64_t Cin, int64_t Cout, int64_t KH,
                       int64_t KW, int64_t stride, int64_t pad_h, int64_t pad_w,
                       int64_t dil_h, int64_t dil_w, int64_t Ho, int64_t Wo);
std::vector<int64_t> conv_wgrad_plan(int64_t M, int64_t Cin, int64_t Cout,
                                     int64_t KH, int64_t KW);
Tensor tr16_probe();

// sgd.hip
void fused_sgd(const Tensor& chunk_table, double lr, double momentum,
               double weight_decay, int64_t dtype_tag);

// heatmap_gt.hip
Tensor heatmap_gt(const Tensor& joints, const c10::optional<Tensor>& mask_all,
                  const Tensor& limb_pairs, int64_t h, int64_t w,
                  int64_t stride, int64_t heat_start, int64_t bkg_start,
                  int64_t num_layers, double sigma, double paf_sigma,
                  double keypoint_thre, double limb_thre, double paf_thre);

// postproc.hip
Tensor peaks_batched(const Tensor& maps, int64_t heat_layers, double thre,
                     int64_t radius, int64_t max_peaks);

// limb_match.hip
Tensor limb_scores(const Tensor& paf, const Tensor& peaks, const Tensor& cand_idx,
                   int64_t mid_num, double thre2);
std::vector<Tensor> peaks_canonical(const Tensor& buf, int64_t n_parts);
std::vector<Tensor> limb_match(const Tensor& maps, const Tensor& peaks,
                               const Tensor& offsets, const Tensor& limbs,
                               int64_t first_limb_plane, int64_t mid_num,
                               double thre2, double connect_ration,
                               int64_t max_part);

// people_assemble.hip
std::vector<Tensor> people_assemble(const Tensor& peaks, const Tensor& offsets,
                                    const Tensor& rows, const Tensor& counts,
                                    const Tensor& limbs, const Tensor& dt_gt,
                                    double len_rate, double connection_tole,
                                    int64_t remove_recon, int64_t max_people);

// ensemble_merge.hip
void ensemble_merge(const Tensor& src, const Tensor& chan_main,
                    const Tensor& chan_flip, const Tensor& ystart,
                    const Tensor& yw, const Tensor& xstart, const Tensor& xw,
                    Tensor& out, double scale, bool accumulate, int64_t cb,
                    int64_t wr, int64_t wc, int64_t span);

// augment.hip
std::vector<Tensor> augment_warp(const Tensor& packed, const Tensor& desc,
                                 int64_t H, int64_t W, int64_t stride,
                                 bool bf16_out);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("bn_v8_geometry", &bn_v8_geometry,
        "debug: [cpb, rpb, rows, grid_y] of the bf16 v8 stats/reduce launch",
        py::arg("M"), py::arg("C"));
  m.def("bn_stats", &bn_stats, "per-channel sum/sumsq of an [M][C] view");
  m.def("bn_finalize", &bn_finalize,
        "mean/invstd/scale/shift epilogue over given (possibly all-reduced) sums");
  m.def("bn_stats_finalize", &bn_stats_finalize,
        "stats + mean/invstd/scale/shift epilogue (+ running-stat update)");
  m.def("bn_act_fwd", &bn_act_fwd, "fused scale/shift (+res) (+leaky)");
  m.def("bn_act_bwd", &bn_act_bwd, "dpre + per-channel reductions");
  m.def("bn_act_bwd_apply", &bn_act_bwd_apply, "BN backward input grad");
  m.def("maxpool2x2_fwd", &maxpool2x2_fwd);
  m.def("maxpool2x2_bwd", &maxpool2x2_bwd);
  m.def("upsample2x_fwd", &upsample2x_fwd);
  m.def("upsample2x_bwd", &upsample2x_bwd);
  m.def("se_reduce", &se_reduce);
  m.def("se_scale", &se_scale);
  m.def("se_gate", &se_gate, "fused GAP-gate: sigmoid(W2@leaky(W1@p+b1)+b2)",
        py::arg("pooled"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("slope"), py::arg("pool_scale") = 1.0);
  m.def("se_layer_grouped", &se_layer_grouped,
        "inference SE layers of independent maps: one launch per stage");
  m.def("focal_l2_fwd", &focal_l2_fwd);
  m.def("focal_l2_bwd", &focal_l2_bwd);
  m.def("conv_mfma_fwd", &conv_mfma_fwd, "MFMA implicit-GEMM conv forward",
        py::arg("x"), py::arg("w_packed"), py::arg("geom"),
        py::arg("scale") = c10::nullopt, py::arg("shift") = c10::nullopt,
        py::arg("residual") = c10::nullopt, py::arg("act") = false,
        py::arg("residual_post") = c10::nullopt,
        py::arg("residual_post2") = c10::nullopt,
        py::arg("x2") = c10::nullopt);
  m.def("conv_mfma_fwd_grouped", &conv_mfma_fwd_grouped,
        "independent MFMA convs in one grouped launch per 8 (+ one combine)",
        py::arg("xs"), py::arg("ws_packed"), py::arg("geom"),
        py::arg("scales"), py::arg("shifts"), py::arg("residuals"),
        py::arg("acts"), py::arg("residual_posts"),
        py::arg("residual_post2s"));
  m.def("conv_mfma_tile_plan", &conv_mfma_tile_plan,
        "debug: [BM, BN, splitk, deep] planned for GEMM extents (M, Cout, K)",
        py::arg("M"), py::arg("Cout"), py::arg("K"));
  m.def("conv_mfma_conv_plan", &conv_mfma_conv_plan,
        "debug: [BM, BN, splitk, deep, gather] planned for conv_mfma_fwd(x, "
        "w_packed, geom); gather 1 = tap-uniform, 0 = generic",
        py::arg("x"), py::arg("w_packed"), py::arg("geom"));
  m.def("pack_conv_weight", &pack_conv_weight,
        "fwd + dgrad weight packs in one kernel",
        py::arg("w"), py::arg("fwd_pack"), py::arg("dgrad_pack") = c10::nullopt);
  m.def("pack_upfold_weight", &pack_upfold_weight,
        "3x3 weight -> four folded 2x2 packs [4][Cout][4*Cin] (nearest-x2 "
        "upsample folded into the conv)",
        py::arg("w"), py::arg("out"));
  m.def("pack_cat_weight", &pack_cat_weight,
        "two 1x1 weights (+ per-channel scales, shifts) -> one [Cout][Ca+Cb] "
        "pack and the fused shift of a two-source 1x1 conv",
        py::arg("wa"), py::arg("wb"), py::arg("scale_a"), py::arg("scale_b"),
        py::arg("shift_a"), py::arg("shift_b"), py::arg("out"),
        py::arg("shift_out"));
  m.def("conv_mfma_upfold_fwd", &conv_mfma_upfold_fwd,
        "conv3x3(nearest_x2(x_low)) + epilogue as four parity 2x2 convs in "
        "one grouped launch",
        py::arg("x_low"), py::arg("packs"), py::arg("geom"),
        py::arg("scale") = c10::nullopt, py::arg("shift") = c10::nullopt,
        py::arg("act") = false, py::arg("residual_post") = c10::nullopt,
        py::arg("residual_post2") = c10::nullopt);
  m.def("conv_mfma_upfold_plan", &conv_mfma_upfold_plan,
        "debug: [BM, BN, splitk, deep] shared by the four parities of an "
        "upfold conv over M_low low-resolution pixels",
        py::arg("M_low"), py::arg("Cout"), py::arg("Cin"));
  m.def("conv_mfma_wgrad", &conv_mfma_wgrad,
        "MFMA implicit-GEMM conv weight gradient (tr16 LDS transpose)");
  m.def("conv_wgrad_plan", &conv_wgrad_plan,
        "debug: [TKD, TCO, waves, elem, kd_cb, chunks, chunk_len, tree group "
        "counts...] planned for a weight gradient with M = N*Ho*Wo",
        py::arg("M"), py::arg("Cin"), py::arg("Cout"), py::arg("KH"),
        py::arg("KW"));
  m.def("tr16_probe", &tr16_probe,
        "debug: ds_read_b64_tr_b16 delivery-map probe");
  m.def("fused_sgd", &fused_sgd);
  m.def("heatmap_gt", &heatmap_gt, "on-device GT heatmap/PAF generation",
        py::arg("joints"), py::arg("mask_all"), py::arg("limb_pairs"),
        py::arg("h"), py::arg("w"), py::arg("stride"), py::arg("heat_start"),
        py::arg("bkg_start"), py::arg("num_layers"), py::arg("sigma"),
        py::arg("paf_sigma"), py::arg("keypoint_thre"), py::arg("limb_thre"),
        py::arg("paf_thre"));
  m.def("limb_scores", &limb_scores);
  m.def("peaks_canonical", &peaks_canonical,
        "peaks_batched buffer -> rows in (channel, y, x) order + channel offsets",
        py::arg("buf"), py::arg("n_parts"));
  m.def("limb_match", &limb_match,
        "per (image, limb): score, filter and greedily match all nA x nB segments",
        py::arg("maps"), py::arg("peaks"), py::arg("offsets"), py::arg("limbs"),
        py::arg("first_limb_plane"), py::arg("mid_num"), py::arg("thre2"),
        py::arg("connect_ration"), py::arg("max_part"));
  m.def("people_assemble", &people_assemble,
        "per image: greedy person assembly over limb_match rows + COCO keypoints",
        py::arg("peaks"), py::arg("offsets"), py::arg("rows"), py::arg("counts"),
        py::arg("limbs"), py::arg("dt_gt"), py::arg("len_rate"),
        py::arg("connection_tole"), py::arg("remove_recon"),
        py::arg("max_people"));
  m.def("peaks_batched", &peaks_batched,
        "fused NMS + centroid refinement over a planar batch, per-image counters",
        py::arg("maps"), py::arg("heat_layers"), py::arg("thre"),
        py::arg("radius"), py::arg("max_peaks"));
  m.def("ensemble_merge", &ensemble_merge,
        "flip-merge + composed bicubic resample of the low-res network output",
        py::arg("src"), py::arg("chan_main"), py::arg("chan_flip"),
        py::arg("ystart"), py::arg("yw"), py::arg("xstart"), py::arg("xw"),
        py::arg("out"), py::arg("scale"), py::arg("accumulate"), py::arg("cb"),
        py::arg("wr"), py::arg("wc"), py::arg("span"));
  m.def("augment_warp", &augment_warp,
        "batched affine warp of ragged uint8 records -> [image NHWC, "
        "mask_miss, mask_all on the stride grid]",
        py::arg("packed"), py::arg("desc"), py::arg("H"), py::arg("W"),
        py::arg("stride"), py::arg("bf16_out"));
}
