"""Every sampler kernel instance the dispatcher can choose, and how a test reaches it (a plain data module).

Each row of ROWS:
  kernel   -- the exact name ctx.last_kernel() reports
  model    -- a shipped model's name, or a dict of util.shaped_model arguments (+ "seed" for its RandomState)
  form     -- "both"        dense init/dyn outputs, no list               (host call, then a device call at a column offset)
              "one"         dyn_bin alone                                  (device call at a column offset)
              "idx"         both dense outputs for an index list           (host call)
              "list"        the event list alone                           (host call, then a device call at a column offset)
              "list+dense"  list and dense outputs                         (host call, then a device call at a column offset)
              "plain"       NO_RESAMPLE | NO_DEDISC | NO_TERMINATOR: dbn_sample.m's list (host call)
              "mixed"       emgpu_sample_dbn_blocks_device, blocks of `model` and the models in "with", one launch (device)
              "bn"          emgpu_sample_bn_host, bn_sample.m (host);  "bn+start": the same with a start grid
  per_step -- EMGPU_TRANSITION_PER_STEP
  env      -- debug variables the library reads once per process (getenv cached in a static): the row runs in a child process

The completeness test (test_instances.py) extracts every kernel name literal and EMGPU_S2_CASE / EMGPU_S2_CASE_W tag from the sources (the
name tables of csrc/emgpu_dispatch.cpp and the case lists of csrc/emgpu_dispatch.h, where the dispatcher keeps them; the single-instance
launchers' own literals) and fails on one that no row reaches and that neither COVERED_ELSEWHERE nor UNREACHABLE lists.
test_dispatch.py predicts every row's kernel on the CPU through emgpu_debug_kernel_choice; test_gpu_instances.py runs it.
"""

RATE_AT_EDGE = 1.0 - 2.0 ** -16               # Bernoulli threshold exactly 0xFFFF0000: RR1 = (R >> 16) + 1 does not fit 16 bits, the
                                              # fast and step2 kernels and the event plans decline it (k_dbn_step, k_dbn_generic take it)
RATE_BELOW_EDGE = 1.0 - 2.0 ** -16 - 2.0 ** -32  # threshold 0xFFFEFFFF, one below: the last rate the fast and step2 kernels take


def shaped(seed, ni, meff, dependent=False, parents=None, rates=None, r=None):
    return dict(seed=seed, ni=ni, meff=tuple(meff), dependent=dependent, parents=parents, rates=rates, r=r)


def rates_on(ni, nd, extra=(), value=0.1, first=None):
    """Rates 0.1 on the nd dynamic variables and the static ones in `extra`; `first` replaces the first dynamic variable's rate."""
    out = [value if (v < nd or v in extra) else 0.0 for v in range(ni)]
    if first is not None:
        out[0] = first
    return out


# ---- the fast branch: three independent dynamic variables, instance <NI,M0,M1,M2> first-fit from kFastShapes
M7_666 = shaped(701, 7, (6, 6, 6))
M7_566 = shaped(702, 7, (5, 6, 6))
M9_666 = shaped(901, 9, (6, 6, 6))   # haa_v1 has seven rated variables (evw / evu_long): this one has three
FAST = {   # shape -> (a model that reaches it, a second one of the same trace shape and labels for the mixed batch, whose run-wide
           # rejection indices idx_L / idx_v / idx_dh then mean the same for both)
    "7,2,2,2": ("blimp_v1", shaped(501, 5, (2, 2, 2)), shaped(502, 5, (1, 2, 2))),
    "7,2,4,2": ("uncor_1200code_v2p1", shaped(703, 7, (2, 4, 2)), shaped(713, 7, (2, 3, 1))),
    "7,2,4,4": ("dueregard_v1", shaped(704, 7, (2, 4, 4)), shaped(714, 7, (1, 3, 4))),
    "7,4,2,4": ("uncor_allcode_rotorcraft_v1", shaped(705, 7, (4, 2, 4)), shaped(715, 7, (3, 1, 3))),
    "7,4,6,4": ("uncor_allcode_fwmulti_v1", shaped(706, 7, (4, 5, 4)), shaped(716, 7, (3, 6, 2))),
    "7,4,6,6": ("uncor_allcode_fwsingle_v1", "uncor_allcode_fwsingle_v1", "uncor_1200only_fwse_v1p2"),
    "7,6,6,6": (M7_666, M7_666, M7_566),
    "9,6,6,6": (M9_666, M9_666, shaped(902, 9, (6, 5, 6))),
}

ROWS = []
for shape, (m, m1, m2) in FAST.items():
    ROWS += [dict(kernel="k_uncor_fast<%s>" % shape, model=m, form="both"),
             dict(kernel="k_uncor_fast_idx<%s>" % shape, model=m, form="idx"),
             dict(kernel="k_uncor_fast_idx<%s>" % shape, model=m, form="one"),
             dict(kernel="k_uncor_fast_ev<%s>" % shape, model=m, form="list+dense"),
             dict(kernel="k_uncor_fast_evu<%s>" % shape, model=m, form="list"),
             dict(kernel="k_uncor_fast_mixed<%s>" % shape, model=m1, form="mixed", with_=[m2])]
ROWS += [
    dict(kernel="k_uncor_fast_evu<7,6,6,6>", model=M7_666, form="plain"),
    dict(kernel="k_uncor_fast_evw<9,6,6,6>", model="haa_v1", form="list+dense"),
    dict(kernel="k_uncor_fast_evu_long<9,6,6,6>", model="haa_v1", form="list"),
    dict(kernel="k_uncor_fast_evu_long<9,6,6,6>", model=shaped(711, 7, (6, 6, 6), rates=[0.3, 0.25, 0.2, 0.0, 0.0, 0.0, 0.0]), form="list"),
]

# ---- k_dbn_step2: the dependent branch (new-value parents, or PER_STEP), and the fast-branch models k_uncor_fast did not take ([frozen])
NOT_A_FAMILY = (0x0421, 0x0100)   # 2 <- new 0 alone: no mask-specific instance
ROWS += [
    dict(kernel="k_dbn_step2<7,3,w4,reg>", model=shaped(721, 6, (2, 3, 3), parents=NOT_A_FAMILY), form="both"),
    dict(kernel="k_dbn_step2<7,3,w8,reg>", model=shaped(722, 6, (5, 4, 6), parents=NOT_A_FAMILY), form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>", model=shaped(723, 7, (2, 5, 3), parents=NOT_A_FAMILY), form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>", model="glider_v1", form="one"),
    dict(kernel="k_dbn_step2<7,3>", model=shaped(724, 7, (3, 4, 2), dependent=True, rates=[0.1, 0.0, 0.1, 0.05, 0, 0, 0]), form="both"),
    dict(kernel="k_dbn_step2<7,3>+rows-by-wave+events", model="glider_v1", form="plain"),
    dict(kernel="k_dbn_step2<9,3,w4,reg>", model=shaped(921, 9, (3, 2, 3), dependent=True), form="both"),
    dict(kernel="k_dbn_step2<9,3,w8,reg>", model=shaped(922, 8, (6, 5, 4), dependent=True), form="both"),
    dict(kernel="k_dbn_step2<9,3,reg>", model=shaped(923, 9, (2, 6, 3), dependent=True), form="both"),
    dict(kernel="k_dbn_step2<9,3,reg>+events", model=shaped(923, 9, (2, 6, 3), dependent=True), form="list+dense"),
    dict(kernel="k_dbn_step2<9,3>", model=shaped(924, 9, (3, 3, 5), dependent=True, rates=[0.0, 0.1, 0.1, 0, 0, 0, 0, 0.05, 0]), form="both"),
    dict(kernel="k_dbn_step2<16,4,w4,reg>", model=shaped(1641, 8, (2, 3, 3, 3), dependent=True), form="both"),
    dict(kernel="k_dbn_step2<16,4,w4,reg>", model="cor_v1", form="one"),
    dict(kernel="k_dbn_step2<16,4,w8,reg>", model=shaped(1642, 8, (4, 5, 6, 4), dependent=True), form="both"),
    dict(kernel="k_dbn_step2<16,4,w8,reg>", model="cor_v2p1_like", form="one"),
    dict(kernel="k_dbn_step2<16,4,reg>", model=shaped(1643, 8, (2, 5, 3, 6), dependent=True), form="both"),
    dict(kernel="k_dbn_step2<16,4,reg>+rows-by-wave+events", model=shaped(1643, 8, (2, 5, 3, 6), dependent=True), form="list"),
    dict(kernel="k_dbn_step2<16,4>", model=shaped(1644, 11, (3, 4, 2), dependent=True), form="both"),
    dict(kernel="k_dbn_step2<16,4,w4,reg>[frozen]", model="littoral_cor_v1", form="both"),
    dict(kernel="k_dbn_step2<16,4>[frozen]", model="littoral_cor_v1", form="one"),
    dict(kernel="k_dbn_step2<16,4>[frozen]", model="weatherballoon_v1", form="both"),
    dict(kernel="k_dbn_step2<16,4>[frozen]+events", model="weatherballoon_v1", form="list+dense"),
    dict(kernel="k_dbn_step2<16,4>[frozen]+rows-by-wave+events", model="weatherballoon_v1", form="list"),
    # the parent-mask instances: "[cor]" (4 variables), the width-specific 3-variable ones (dense outputs only), the per-variable width ones
    dict(kernel="k_dbn_step2<16,4,w4,reg>[cor]", model="cor_v1", form="both"),
    dict(kernel="k_dbn_step2<16,4,w8,reg>[cor]", model="cor_v2p1_like", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[chain,w884]", model="glider_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[chain,w888]", model="paraglider_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[2<-1,w444]", model="littoral_uncor_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[2<-1,w884]", model="paramotor_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[2<-1,w484]", model="skydiving_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[1<-0,2<-0,w888]", model="fai1_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[1<-0,2<-0,w848]", model="fai5_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[1<-0,2<-0,w848]", model=shaped(731, 5, (6, 3, 4), parents=(0x0421, 0x0110)), form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[2<-0,1,w844]", model="uncor_1200code_v1", form="both"),
    dict(kernel="k_dbn_step2<7,3,reg>[per-step,w484]", model="uncor_1200code_v2p1", form="both", per_step=True),
    dict(kernel="k_dbn_step2<7,3,reg>[per-step,w888]", model="uncor_allcode_fwsingle_v1", form="both", per_step=True),
    dict(kernel="k_dbn_step2<7,3,reg>[chain]+events", model="glider_v1", form="list+dense"),
    dict(kernel="k_dbn_step2<7,3,reg>[2<-1]+events", model="littoral_uncor_v1", form="list+dense"),
    dict(kernel="k_dbn_step2<7,3,reg>[1<-0,2<-0]+events", model="fai5_v1", form="list+dense"),
    dict(kernel="k_dbn_step2<7,3,reg>[1<-0,2<-0]+rows-by-wave+events", model="fai5_v1", form="list"),
    dict(kernel="k_dbn_step2<7,3,reg>[2<-0,1]+events", model="uncor_1200code_v1", form="list+dense"),
    dict(kernel="k_dbn_step2<7,3,reg>[per-step]+events", model="uncor_1200code_v2p1", form="list+dense", per_step=True),
    dict(kernel="k_dbn_step2<7,3,reg>[per-step]+rows-by-wave+events", model="uncor_allcode_fwsingle_v1", form="list", per_step=True),
]

# ---- k_dbn_step: the dependent branch when step2 declines (a dynamic variable's rate at or above 1 - 2^-16); _lds: tables staged in LDS
STEP_MODELS = {"7,3": shaped(741, 6, (2, 3, 3), dependent=True, rates=rates_on(6, 3, first=RATE_AT_EDGE)),
               "9,3": shaped(941, 9, (4, 3, 6), dependent=True, rates=rates_on(9, 3, first=RATE_AT_EDGE)),
               "16,4": shaped(1645, 8, (3, 3, 2, 5), dependent=True, rates=rates_on(8, 4, first=RATE_AT_EDGE))}
for s, m in STEP_MODELS.items():
    ROWS += [dict(kernel="k_dbn_step<%s,8,lds>" % s, model=m, form="both"),
             dict(kernel="k_dbn_step<%s,8>" % s, model=m, form="both", env={"EMGPU_DEBUG_STEP_NO_LDS": "1"})]

# ---- k_dbn_generic: a rate of exactly 1 (threshold 0xFFFFFFFF) leaves no other kernel; index lists of dependent models
ROWS += [
    dict(kernel="k_dbn_generic<7,3,4>", model=shaped(751, 6, (2, 3, 3), dependent=True, rates=rates_on(6, 3, first=1.0)), form="both"),
    dict(kernel="k_dbn_generic<7,3,4>", model="fai5_v1", form="idx"),
    dict(kernel="k_dbn_generic<7,3,7>", model=shaped(752, 7, (3, 3, 3), dependent=True, rates=rates_on(7, 3, extra=(3, 4, 5), first=1.0)), form="both"),
    dict(kernel="k_dbn_generic<9,3,9>", model=shaped(951, 9, (3, 3, 3), dependent=True, rates=rates_on(9, 3, extra=(3, 4, 5, 6, 7), first=1.0)), form="both"),
    dict(kernel="k_dbn_generic<16,4,4>", model=shaped(1651, 8, (2, 2, 3, 3), dependent=True, rates=rates_on(8, 4, first=1.0)), form="both"),
    dict(kernel="k_dbn_generic<16,4,4>", model="cor_v1", form="idx"),
    dict(kernel="k_dbn_generic<16,4,16>", model=shaped(1652, 8, (2, 2, 3, 3), dependent=True, rates=rates_on(8, 4, extra=(5, 6), first=1.0)), form="both"),
]

# ---- k_bn: bn_sample.m (the initial network alone)
ROWS += [
    dict(kernel="k_bn<8>", model=shaped(761, 8, (2, 2, 2)), form="bn"),
    dict(kernel="k_bn<8>+start", model=shaped(761, 8, (2, 2, 2)), form="bn+start"),
    dict(kernel="k_bn<16>", model=shaped(1661, 12, (2, 2, 2)), form="bn"),
    dict(kernel="k_bn<16>+start", model=shaped(1661, 12, (2, 2, 2)), form="bn+start"),
]

# Single-instance kernels outside the sampler: the test that asserts the name and checks the kernel against the oracle.
COVERED_ELSEWHERE = {
    "k_sample2track<planar>": "tests.test_gpu_parity::test_sample2track_kernel_matches_oracle",
    "k_sample2track<dense>": "tests.test_gpu_parity::test_sample2track_consumes_the_dense_trace_on_the_device",
    "k_terminal_propagate<35,6,4>": "tests.test_gpu_parity::test_fused_terminal_call_matches_oracle",
    "k_uncor_track<fastbank>": "tests.test_gpu_parity::test_uncor_track_matches_oracle",
}

# Names the sources carry that no dispatch can choose, each with the reason.
UNREACHABLE = {}

# ---- eligibility edges: the same model family on both sides of each limit where the dispatcher changes kernel
EDGES = [
    # (what, row on the low side, row on the high side, the one shaped_model argument in which the two sides differ)
    ("meff 6 vs 7",
     dict(kernel="k_uncor_fast<7,6,6,6>", model=shaped(771, 7, (6, 6, 6), r=[8, 8, 8, 3, 3, 3, 3]), form="both"),
     dict(kernel="k_dbn_generic<7,3,4>", model=shaped(771, 7, (7, 6, 6), r=[8, 8, 8, 3, 3, 3, 3]), form="both"),   # no padded form: step2 declines too
     "meff"),
    ("d_nb 16 vs 17 (15 vs 16 bins)",
     dict(kernel="k_uncor_fast<7,2,2,2>", model=shaped(772, 7, (2, 2, 2), r=[15, 4, 4, 3, 3, 3, 3]), form="both"),
     dict(kernel="k_dbn_generic<7,3,4>", model=shaped(772, 7, (2, 2, 2), r=[16, 4, 4, 3, 3, 3, 3]), form="both"), "r"),
    ("rate 1 - 2^-16 - 2^-32 vs 1 - 2^-16 on a dynamic variable, fast branch",
     dict(kernel="k_uncor_fast<7,2,4,4>", model=shaped(773, 7, (2, 3, 3), rates=rates_on(7, 3, first=RATE_BELOW_EDGE)), form="both"),
     dict(kernel="k_dbn_generic<7,3,4>", model=shaped(773, 7, (2, 3, 3), rates=rates_on(7, 3, first=RATE_AT_EDGE)), form="both"), "rates"),
    ("rate 1 - 2^-16 - 2^-32 vs 1 - 2^-16 on a dynamic variable, dependent branch",
     dict(kernel="k_dbn_step2<7,3,w4,reg>", model=shaped(774, 7, (2, 3, 3), parents=NOT_A_FAMILY, rates=rates_on(7, 3, first=RATE_BELOW_EDGE)), form="both"),
     dict(kernel="k_dbn_step<7,3,8,lds>", model=shaped(774, 7, (2, 3, 3), parents=NOT_A_FAMILY, rates=rates_on(7, 3, first=RATE_AT_EDGE)), form="both"), "rates"),
    ("nact 5 vs 6 (ev_plan_ok: 8 - nd), list and dense",
     dict(kernel="k_uncor_fast_ev<7,4,6,6>", model=shaped(775, 7, (4, 6, 6), rates=rates_on(7, 3, extra=(3, 4))), form="list+dense"),
     dict(kernel="k_uncor_fast_evw<9,6,6,6>", model=shaped(775, 7, (4, 6, 6), rates=rates_on(7, 3, extra=(3, 4, 5))), form="list+dense"), "rates"),
    ("rate 1 - 2^-16 - 2^-32 vs 1 - 2^-16 on a static variable, list and dense (ev_plan_ok)",
     dict(kernel="k_uncor_fast_ev<7,2,4,4>", model=shaped(779, 7, (2, 3, 3), rates=[0.1, 0.1, 0.1, RATE_BELOW_EDGE, 0, 0, 0]), form="list+dense"),
     dict(kernel="k_dbn_generic<7,3,4>", model=shaped(779, 7, (2, 3, 3), rates=[0.1, 0.1, 0.1, RATE_AT_EDGE, 0, 0, 0]), form="list+dense"), "rates"),
    ("rate 1 - 2^-16 - 2^-32 vs 1 - 2^-16 on a static variable, list alone (ev_plan_wide_ok)",
     dict(kernel="k_uncor_fast_evu_long<9,6,6,6>", model=shaped(779, 7, (2, 3, 3), rates=[0.1, 0.1, 0.1, RATE_BELOW_EDGE, 0, 0, 0]), form="list"),
     dict(kernel="k_dbn_generic<7,3,4>", model=shaped(779, 7, (2, 3, 3), rates=[0.1, 0.1, 0.1, RATE_AT_EDGE, 0, 0, 0]), form="list"), "rates"),
    ("nact 5 vs 6 (step2 events, three-variable instance: the same limit as ev_plan_ok's 8 - nd)",
     dict(kernel="k_dbn_step2<7,3,w4,reg>+events", model=shaped(780, 7, (2, 3, 3), parents=NOT_A_FAMILY, rates=rates_on(7, 3, extra=(3, 4))), form="list+dense"),
     dict(kernel="k_dbn_generic<7,3,7>", model=shaped(780, 7, (2, 3, 3), parents=NOT_A_FAMILY, rates=rates_on(7, 3, extra=(3, 4, 5))), form="list+dense"), "rates"),
    ("nact 4 vs 5 (step2 events, four-variable instance)",
     dict(kernel="k_dbn_step2<16,4>+events", model=shaped(1171, 11, (3, 3, 3), dependent=True, rates=rates_on(11, 3, extra=(5,))), form="list+dense"),
     dict(kernel="k_dbn_generic<16,4,16>", model=shaped(1171, 11, (3, 3, 3), dependent=True, rates=rates_on(11, 3, extra=(5, 6))), form="list+dense"), "rates"),
    ("nact 12 vs 13 (step2 list alone, four-variable instance; ev_plan_wide_ok holds both)",
     dict(kernel="k_dbn_step2<16,4>+rows-by-wave+events", model=shaped(1371, 13, (3, 3, 3), dependent=True, rates=[0.02] * 12 + [0.0]), form="list"),
     dict(kernel="k_dbn_generic<16,4,16>", model=shaped(1371, 13, (3, 3, 3), dependent=True, rates=[0.02] * 13), form="list"), "rates"),
    # (ev_plan_wide_ok's own limit, 16 - nd rated variables, never binds: a fast-branch list needs ni <= 9, and step2 stops at 12 or 13 first)
    ("nact 12 vs 13 (step2 list alone, frozen instance)",
     dict(kernel="k_dbn_step2<16,4>[frozen]+rows-by-wave+events", model=shaped(1471, 14, (2, 2), rates=[0.02] * 12 + [0.0] * 2), form="list"),
     dict(kernel="k_dbn_generic<16,4,16>", model=shaped(1471, 14, (2, 2), rates=[0.02] * 13 + [0.0]), form="list"), "rates"),
    ("ni 7 vs 8",
     dict(kernel="k_uncor_fast<7,6,6,6>", model=shaped(776, 7, (6, 6, 6)), form="both"),
     dict(kernel="k_uncor_fast<9,6,6,6>", model=shaped(776, 8, (6, 6, 6)), form="both"), "ni"),
    ("ni 9 vs 10",
     dict(kernel="k_uncor_fast<9,6,6,6>", model=shaped(777, 9, (3, 3, 3)), form="both"),
     dict(kernel="k_dbn_step2<16,4>[frozen]", model=shaped(777, 10, (3, 3, 3)), form="both"), "ni"),
    ("every dynamic variable rated vs one rate 0 (reg)",
     dict(kernel="k_dbn_step2<7,3,w8,reg>", model=shaped(778, 7, (4, 5, 6), parents=NOT_A_FAMILY), form="both"),
     dict(kernel="k_dbn_step2<7,3>", model=shaped(778, 7, (4, 5, 6), parents=NOT_A_FAMILY, rates=[0.1, 0.1, 0.0, 0, 0, 0, 0]), form="both"), "rates"),
]
