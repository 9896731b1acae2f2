// Private to libhavoc_mi355x.so: the ONE declaration of every launcher, workspace size and limit that crosses a file boundary; every .hip file that defines or calls
// one includes it, so a definition that drifts from its declaration does not compile and a declaration without a definition does not link.  Job tables, records and
// layouts carry their public record type; sample planes (element type by S), workspaces and the records of search/search_abi.h stay void pointers.
#pragma once

#include "common.h"

namespace havoc_gpu {
hipError_t launch_sad(hipStream_t, int S, const void *, long, const void *, long, const havoc_mi355x_pair_job *, int, int32_t *);
hipError_t launch_sad4(hipStream_t, int S, const void *, long, const void *, long, const havoc_mi355x_sad4_job *, int, int32_t *);
hipError_t launch_sad4_runs(hipStream_t, int S, const void *, long, const void *, long, const havoc_mi355x_sad4_job *, int, const havoc_mi355x_sad4_run *, int, int32_t *);
hipError_t launch_sad_surface(hipStream_t, int S, int range, int maxw, int maxh, const void *, long, const void *, long, const havoc_mi355x_surface_job *, int, int32_t *);
hipError_t launch_ssd(hipStream_t, int S, const void *, long, const void *, long, const havoc_mi355x_pair_job *, int, uint32_t *);
hipError_t launch_satd(hipStream_t, int S, int maxw, int maxh, const void *, long, const void *, long, const havoc_mi355x_pair_job *, int, int32_t *);
hipError_t launch_satd_multi(hipStream_t, int S, int maxw, int maxh, const void *, long, const void *, long, const havoc_mi355x_satd_multi_job *, int, int32_t *);
hipError_t launch_ssd_linear(hipStream_t, const uint8_t *, const uint8_t *, int, int32_t *);
hipError_t launch_pad_block(hipStream_t, int S, void *, long, int, int, long, int, int, int, int, int);
hipError_t launch_derive_bs(hipStream_t, const havoc_mi355x_cell *, long, int, int, int8_t *, uint8_t *);
hipError_t launch_deblock(hipStream_t, int S, int bd, void *, long, void *, void *, long, int, int, const int8_t *, const uint8_t *, int, int, int, int);
hipError_t launch_interp_planes(hipStream_t, int S, int bd, void *, long, const void *, long, int, int, int, int);
hipError_t launch_pred_uni(hipStream_t, int S, int taps, int bd, int maxw, int maxh, void *, long, const void *, long, const havoc_mi355x_pred_uni_job *, int);
hipError_t launch_pred_bi(hipStream_t, int S, int taps, int bd, int maxw, int maxh, void *, long, const void *, long, const havoc_mi355x_pred_bi_job *, int);
hipError_t launch_pred_uni_classes(hipStream_t, int S, int taps, int bd, void *, long, const void *, long, const havoc_mi355x_pred_uni_job *, const int count[4]);
hipError_t launch_pred_bi_classes(hipStream_t, int S, int taps, int bd, void *, long, const void *, long, const havoc_mi355x_pred_bi_job *, const int count[4]);
hipError_t launch_subtract_bi(hipStream_t, int S, int bd, void *, long, const void *, long, const void *, long, const havoc_mi355x_subtract_bi_job *, int);
hipError_t launch_subpel_satd(hipStream_t, int S, int taps, int bd, int maxw, int maxh, const void *, long, const void *, long, const havoc_mi355x_pred_uni_job *, int,
                              int32_t *);
hipError_t launch_intra(hipStream_t, int S, int log2, int bd, void *, long, const void *, const havoc_mi355x_intra_job *, int);
hipError_t launch_intra_satd35(hipStream_t, int S, int log2, int bd, const void *, long, const void *, const havoc_mi355x_intra_search_job *, int, int32_t *);
hipError_t launch_transform(hipStream_t, int bd, int log2, int tr, int16_t *, const int16_t *, long, const havoc_mi355x_tu_job *, int);
hipError_t launch_inverse_transform(hipStream_t, int mode, int bd, int log2, int tr, void *, long, const void *, long, int16_t *, const int16_t *,
                                    const havoc_mi355x_tu_job *, int);
hipError_t launch_level_stats(hipStream_t, const int16_t *, const int32_t *, int, int32_t *);
hipError_t launch_quantize(hipStream_t, int16_t *, const int16_t *, const havoc_mi355x_quant_job *, int, int32_t *);
hipError_t launch_quantize_inverse(hipStream_t, int16_t *, const int16_t *, const havoc_mi355x_quant_job *, int);
hipError_t launch_quantize_reconstruct(hipStream_t, int log2, uint8_t *, long, const uint8_t *, long, const int16_t *, const havoc_mi355x_tu_job *, int);
hipError_t launch_residual(hipStream_t, int S, int16_t *, long, const int32_t *, const void *, long, const void *, long, const havoc_mi355x_pair_job *, int);
hipError_t launch_tu_forward(hipStream_t, int S, int bd, int log2, int tr, int16_t *, const void *, long, const void *, long, const havoc_mi355x_tu_fused_job *, int);
hipError_t launch_tu_forward_scan(hipStream_t, int S, int bd, int log2, int16_t *, const void *, long, const void *, long, const havoc_mi355x_tu_fused_job *, int,
                                  const havoc_mi355x_rdoq_job *, int16_t *, void *);
hipError_t launch_intra_measure(hipStream_t, int S, int bd, int log2, int16_t *, int16_t *, int32_t *, void *, uint32_t *, const void *, long, const void *, long,
                                const havoc_mi355x_tu_fused_job *, int, int);
hipError_t launch_tu_reconstruct(hipStream_t, int S, int bd, int log2, int tr, int scale, int shift, void *, long, const void *, long, const void *, long, const int16_t *,
                                 const havoc_mi355x_tu_fused_job *, int, uint32_t *);
size_t rdoq_workspace_bytes(int njobs);
hipError_t launch_rdoq(hipStream_t, int bd, int log2, int16_t *, const int16_t *, const uint8_t *, const havoc_mi355x_rdoq_job *, int, int32_t *, void *);
hipError_t launch_rdoq_prescanned(hipStream_t, int bd, int log2, int16_t *, const int16_t *, const uint8_t *, const havoc_mi355x_rdoq_job *, int, int32_t *, void *);
hipError_t launch_residual_rate(hipStream_t, int log2, const int16_t *, const uint8_t *, const havoc_mi355x_residual_rate_job *, int, int64_t *, uint8_t *);
hipError_t launch_intra_rate(hipStream_t, int log2, const int16_t *, const uint8_t *, const uint8_t *, const havoc_mi355x_intra_rate_job *, int, int64_t *, uint8_t *, uint8_t *);
hipError_t launch_tree_rate(hipStream_t, int log2Cb, int depth, const int16_t *, const int16_t *, const uint8_t *, const uint8_t *, const havoc_mi355x_tree_rate_job *, int, int64_t *,
                            uint32_t *, uint8_t *, uint8_t *);
hipError_t launch_pu_rate(hipStream_t, const uint8_t *, const havoc_mi355x_pu_rate_job *, int, const havoc_mi355x_pu_slice *, int64_t *, uint8_t *);
hipError_t launch_pu_decide(hipStream_t, const int32_t *, const int32_t *, int, const int64_t *, const int32_t *, const int32_t *, const int32_t *, int32_t, const uint8_t *,
                            int64_t *, int32_t *, int64_t *, uint8_t *);
hipError_t launch_cu_close(hipStream_t, const uint8_t *, const uint8_t *, const uint8_t *, const int64_t *, const havoc_mi355x_rqt_choice *, const havoc_mi355x_rqt_tree_choice *,
                           const int64_t *, const int32_t *, const havoc_mi355x_cu_close_job *, int, int, int32_t, havoc_mi355x_cu_choice *, uint8_t *, uint8_t *);
hipError_t launch_unit_pred_ssd(hipStream_t, int S, const void *, long, const void *, long, const void *, long, const void *, long, const havoc_mi355x_pred_ssd_job *, int,
                                int32_t *);
hipError_t launch_unit_pred_select(hipStream_t, int S, const void *, const void *, void *, long, void *, long, const int32_t *, const int32_t *, const int64_t *,
                                   const havoc_mi355x_pred_select_job *, int, int64_t *, int32_t *);
size_t cqt_decide_workspace_bytes(int nctus);
hipError_t launch_cqt_decide(hipStream_t, int width, int height, int ctbLog2, int minCbLog2, int flags, const uint8_t *, const int32_t *, const havoc_mi355x_cu_choice *, int,
                             void *work, havoc_mi355x_cqt_ctu *, havoc_mi355x_cqt_node *, int8_t *, uint8_t *);
hipError_t launch_cqt_commit(hipStream_t, const havoc_mi355x_cqt_commit_args &);
hipError_t launch_cqt_block_cells(hipStream_t, int width, int height, int minCbLog2, int qp, int dpb0, int dpb1, const havoc_mi355x_cqt_cell *, havoc_mi355x_cell *,
                                  long stride);
hipError_t launch_cqt_motion_store(hipStream_t, int width, int height, int minCbLog2, int refPoc0, int refPoc1, const havoc_mi355x_cqt_cell *, havoc_mi355x_col_cell *);
hipError_t launch_temporal_candidates(hipStream_t, const havoc_mi355x_temporal_params &, const havoc_mi355x_col_cell *, long stride, const void *pus, int n,
                                      havoc_mi355x_temporal_cand *);
hipError_t launch_cqt_merge_lists(hipStream_t, const havoc_mi355x_merge_params &, const havoc_mi355x_cqt_cell *, const void *pus, int n,
                                  const havoc_mi355x_temporal_cand *temporal, havoc_mi355x_merge_list *);
hipError_t launch_intra_order(hipStream_t, const int32_t *, const havoc_mi355x_intra_mpm *, int, int32_t, int32_t *, int32_t *, int32_t *, int32_t *);
hipError_t launch_intra_expand(hipStream_t, const havoc_mi355x_intra_search_job *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, int, int, int, int, int,
                               int, int, int, havoc_mi355x_intra_job *, havoc_mi355x_tu_fused_job *, havoc_mi355x_rdoq_job *, int32_t *, int32_t *);
hipError_t launch_intra_decide(hipStream_t, const havoc_mi355x_intra_mpm *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const uint32_t *,
                               const int32_t *, const havoc_mi355x_tu_fused_job *, int, int, int32_t, havoc_mi355x_intra_choice *, havoc_mi355x_tu_fused_job *,
                               const int64_t *rates);
hipError_t launch_intra_rate_jobs(hipStream_t, const havoc_mi355x_intra_mpm *, const int32_t *, const int32_t *, const int32_t *, const havoc_mi355x_rdoq_job *, int, int,
                                  havoc_mi355x_intra_rate_job *);
hipError_t launch_intra_fill_spare(hipStream_t, const int32_t *, int, int, havoc_mi355x_intra_job *, havoc_mi355x_tu_fused_job *, havoc_mi355x_rdoq_job *, int32_t *, int32_t *);
hipError_t launch_intra_gather(hipStream_t, int S, const havoc_mi355x_intra_chain_layout *, const void *, const int32_t *, const uint8_t *,
                               const havoc_mi355x_intra_chain_part *, int, const havoc_mi355x_intra_search_job *, void *, havoc_mi355x_intra_mpm *);
hipError_t launch_intra_commit(hipStream_t, int S, const havoc_mi355x_intra_chain_layout *, void *, uint8_t *, const havoc_mi355x_intra_chain_part *, int, const void *,
                               const int32_t *, int);
hipError_t launch_rqt_decide(hipStream_t, const havoc_mi355x_rqt_unit *, int, const int32_t *, const int32_t *, const havoc_mi355x_rqt_size sizes[4], long, int, int, int32_t,
                             havoc_mi355x_rqt_choice *, const int64_t *const *rates);
hipError_t launch_rqt_decide_tree(hipStream_t, const havoc_mi355x_rqt_unit *, int, const int32_t *, const int32_t *, const havoc_mi355x_rqt_size sizes[4],
                                  const havoc_mi355x_rqt_size csizes[4], const havoc_mi355x_rqt_chroma_at *, const int64_t *, const uint32_t *, long, int, int, long, long, int, int,
                                  int32_t, havoc_mi355x_rqt_choice *, havoc_mi355x_rqt_tree_choice *);
hipError_t launch_rqt_decide_units(hipStream_t, const havoc_mi355x_rqt_unit *, int, const int32_t *, const int32_t *, const havoc_mi355x_rqt_size sizes[4],
                                   const havoc_mi355x_rqt_size csizes[4], const havoc_mi355x_rqt_chroma_at *, const int64_t *, const uint32_t *, int32_t,
                                   havoc_mi355x_rqt_choice *, havoc_mi355x_rqt_tree_choice *);
hipError_t launch_block_cells(hipStream_t, int, int, int, int, const int16_t *, const havoc_mi355x_rqt_unit *, const havoc_mi355x_rqt_choice *, int, havoc_mi355x_cell *, bool);
hipError_t launch_merge_decide(hipStream_t, const int32_t *, const int32_t *, const int32_t *, int, int64_t, int64_t *, int32_t *);
hipError_t launch_merge_jobs(hipStream_t, const havoc_mi355x_field_layout *, const int16_t *, const int32_t *, const int32_t *, int, int, havoc_mi355x_pred_bi_job *,
                             havoc_mi355x_pred_bi_job *, havoc_mi355x_pred_bi_job *, int16_t *);
hipError_t launch_pred_jobs(hipStream_t, const havoc_mi355x_field_layout *, const int16_t *, int, const int32_t *, const int32_t *, int, int, int, const int32_t *,
                            havoc_mi355x_pred_uni_job *);
size_t search_workspace_bytes(int width, int height);
hipError_t launch_search_list(hipStream_t, int S, const havoc_mi355x_search_params *, const void *, long, long, const void *, long, long, const void *, long, long, const void *,
                              int, void *);
hipError_t launch_search_bi_list(hipStream_t, int S, const havoc_mi355x_search_params *, const void *, long, long, const void *, long, long, const void *, long, long, const void *,
                                 long, const void *, const int16_t *, int, void *);
hipError_t launch_search_picture_uni(hipStream_t, int S, const havoc_mi355x_search_params *, const int64_t *, const void *, long, long, const void *, const long *, long,
                                     const void *, long, const long *, const void *, const int32_t *, int, int, int, void *, void *, int16_t *, void *, int, const int32_t *,
                                     const void *temporal);
hipError_t launch_search_walk_temporal(hipStream_t, int S, const void *searchArgs, const void *temporal, int stepLaunches);
hipError_t launch_search_wait_rows(hipStream_t, const void *, int, int, int, int *);
hipError_t launch_sao_stats(hipStream_t, int S, int bd, const void *, long, const void *, long, const havoc_mi355x_sao_stats_job *, int, int64_t *);
hipError_t launch_sao_band_chroma(hipStream_t, int S, int bd, const void *, long, const void *, long, const havoc_mi355x_sao_chroma_job *, int, int64_t *);
hipError_t launch_sao_filter(hipStream_t, int S, int bd, void *, long, const void *, long, const havoc_mi355x_sao_job *, int);
size_t sao_workspace_bytes(int nctus);
hipError_t launch_sao_estimate(hipStream_t, int S, int bd, double lambda, int flags, const void *, const void *, long, long, const void *, const void *, long, long,
                               void *, void *, long, long, const havoc_mi355x_sao_ctu *, int, void *, havoc_mi355x_sao_params *);
size_t sao_decide_workspace_bytes(int nctus);
int sao_decide_max_row();
hipError_t launch_sao_decide(hipStream_t, int S, int bd, long long lambda, int flags, const void *, const void *, long, long, const void *, const void *, long, long,
                             void *, void *, long, long, const havoc_mi355x_sao_ctu *, int, int, const havoc_mi355x_sao_params *, int, int, void *, havoc_mi355x_sao_decision *);
hipError_t launch_sao_apply(hipStream_t, int S, int bd, int flags, int width, int height, int log2, const void *, const void *, const void *, long, long,
                            void *, void *, void *, long, long, const havoc_mi355x_sao_decision *, const havoc_mi355x_sao_bounds *, const int8_t *, long);
} // namespace havoc_gpu
