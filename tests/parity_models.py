"""The shipped models test_gpu_parity.py walks, by the branch of dbn_sample.m they take (a plain data module: test_dispatch.py predicts the
kernels of the same lists without a GPU)."""

FAST_MODELS = ["uncor_1200code_v2p1", "uncor_1200only_fwse_v1p2", "uncor_1200exclude_rotorcraft_v1p2",
               "uncor_allcode_fwmulti_v1", "dueregard_v1", "haa_v1", "blimp_v1"]
DEP_MODELS = ["uncor_1200code_v1", "littoral_uncor_v1", "glider_v1", "paraglider_v1", "fai1_v1", "paramotor_v1", "skydiving_v1"]
