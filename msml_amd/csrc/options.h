// The library's switches: ONE table, read from the environment once (options.hip), changed afterwards only through
// msml_set_option (msml_hip.h).  No other file in csrc/ looks at the environment; a site reads a field:
// `if (msml_opt().no_fast_conv)`.
#pragma once
#include <atomic>

// Parse kinds -- the rules the sites had when each parsed its own variable:
//   PRESENT  1 when the variable exists, whatever its text (MSML_NO_FAST_CONV=0 switches the fast kernels OFF)
//   INT      atoi of the text when the variable exists, the default otherwise
//   LONG     atol of the text when the variable exists, the default otherwise
//   NOT0     0 when the text parses (atoi) to 0, 1 otherwise and when the variable is absent
//   NOT0CH   0 when the first character is '0', 1 otherwise and when absent (MSML_PW_CONV: "all" and "1" are on)
// X(field, environment name, kind, default)
#define MSML_OPTIONS(X)                                               \
  /* conv_igemm.hip: every specialised conv kernel off */             \
  X(no_fast_conv, "MSML_NO_FAST_CONV", PRESENT, 0)                    \
  /* conv_fast.hip */                                                 \
  X(conv_no_one_stage, "MSML_CONV_NO_ONE_STAGE", PRESENT, 0)          \
  X(conv_no_parity, "MSML_CONV_NO_PARITY", PRESENT, 0)                \
  X(conv_big_tile, "MSML_CONV_BIG_TILE", INT, 0)                      \
  X(conv_no_small_m, "MSML_CONV_NO_SMALL_M", PRESENT, 0)              \
  X(conv_small_m_wgs, "MSML_CONV_SMALL_M_WGS", LONG, 200)             \
  X(no_x3_small_m, "MSML_NO_X3_SMALL_M", PRESENT, 0)                  \
  /* conv_pw.hip */                                                   \
  X(pw_conv, "MSML_PW_CONV", NOT0CH, 1)                               \
  X(pw_wgs_per_cu, "MSML_PW_WGS_PER_CU", INT, 4)                      \
  X(pw_upw, "MSML_PW_UPW", INT, 1)                                    \
  /* conv_halo.hip */                                                 \
  X(no_halo_conv, "MSML_NO_HALO_CONV", PRESENT, 0)                    \
  X(halo_wide_only, "MSML_HALO_WIDE_ONLY", PRESENT, 0)                \
  X(halo_no_one_slab, "MSML_HALO_NO_ONE_SLAB", PRESENT, 0)            \
  X(halo_persist, "MSML_HALO_PERSIST", NOT0, 1)                       \
  X(halo_m16, "MSML_HALO_M16", INT, 2)                                \
  X(bnin_acc_persist, "MSML_BNIN_ACC_PERSIST", NOT0, 1)               \
  /* conv_halo2.hip */                                                \
  X(no_halo2_conv, "MSML_NO_HALO2_CONV", PRESENT, 0)                  \
  X(no_halo2_mosaic, "MSML_NO_HALO2_MOSAIC", PRESENT, 0)              \
  X(no_halo2_s2, "MSML_NO_HALO2_S2", PRESENT, 0)                      \
  X(no_halo2_x3, "MSML_NO_HALO2_X3", PRESENT, 0)                      \
  /* conv_ws.hip, conv_s2r.hip, conv_r32.hip, conv_line.hip, conv_d4.hip */ \
  X(no_ws_conv, "MSML_NO_WS_CONV", PRESENT, 0)                        \
  X(ws_m16, "MSML_WS_M16", NOT0, 1)                                   \
  X(no_s2r_conv, "MSML_NO_S2R_CONV", PRESENT, 0)                      \
  X(no_s2r_stride1, "MSML_NO_S2R_STRIDE1", PRESENT, 0)                \
  X(no_s2r_x3, "MSML_NO_S2R_X3", PRESENT, 0)                          \
  X(no_r32_conv, "MSML_NO_R32_CONV", PRESENT, 0)                      \
  X(r32_rows, "MSML_R32_ROWS", INT, 0)                                \
  X(no_line_conv, "MSML_NO_LINE_CONV", PRESENT, 0)                    \
  X(no_d4_conv, "MSML_NO_D4_CONV", PRESENT, 0)                        \
  /* conv_wgrad.hip, wgrad_halo.hip, wgrad_n32.hip, fc_wgrad.hip */   \
  X(no_fast_wgrad, "MSML_NO_FAST_WGRAD", PRESENT, 0)                  \
  X(no_fast_wgrad_group, "MSML_NO_FAST_WGRAD_GROUP", PRESENT, 0)      \
  X(wgrad_no_multitap, "MSML_WGRAD_NO_MULTITAP", PRESENT, 0)          \
  X(wgrad_multitap_wide, "MSML_WGRAD_MULTITAP_WIDE", INT, 128)        \
  X(wgrad_wgs, "MSML_WGRAD_WGS", LONG, 0)                             \
  X(wgrad_minchunk, "MSML_WGRAD_MINCHUNK", LONG, 256)                 \
  X(no_halo_wgrad, "MSML_NO_HALO_WGRAD", PRESENT, 0)                  \
  X(wgrad_halo_wide_min, "MSML_WGRAD_HALO_WIDE_MIN", INT, 128)        \
  X(wgrad_halo_no_pair7, "MSML_WGRAD_HALO_NO_PAIR7", PRESENT, 0)      \
  X(wgrad_halo_no_remap, "MSML_WGRAD_HALO_NO_REMAP", PRESENT, 0)      \
  X(no_n32_wgrad, "MSML_NO_N32_WGRAD", PRESENT, 0)                    \
  X(no_fc_wgrad, "MSML_NO_FC_WGRAD", PRESENT, 0)                      \
  /* bn.hip, layout.hip */                                            \
  X(red_ppt, "MSML_RED_PPT", LONG, 16)                                \
  X(ew_grid, "MSML_EW_GRID", LONG, 768)                               \
  X(no_stem_lds, "MSML_NO_STEM_LDS", PRESENT, 0)

// One switch: a relaxed atomic, so msml_set_option on one thread and a launch on another (the autograd thread) is
// defined behaviour; a relaxed load is a plain load on the host.
struct MsmlOption {
  std::atomic<long> v;
  operator long() const { return v.load(std::memory_order_relaxed); }
};

struct MsmlOptions {
#define X(field, env, kind, def) MsmlOption field{{def}};
  MSML_OPTIONS(X)
#undef X
};

// The table, filled from the environment on first use.
const MsmlOptions& msml_opt();
