"""Cost of the batch sampler's boundary kernels beyond 64 landmarks (k_fbb_segment on the band against the triangle): ten f64
sweeps of 2 000 utterances, D = 8, K = 10, fixed-variance components, window 6, 8 x 8 blocks.  From the repository root:

    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python tools/prof_fbb_long.py ragged|n150|n64 [standard|viterbi]

ragged: 3..150 landmarks (the corpus family of tests/fbgmm_long.py); n150 / n64: every utterance that long.  The kernels'
rows of OUT/.../*_kernel_stats.csv are the figures of profiles/README.md (80 launches of 250 utterances each)."""
import os, random, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from segmentalist_amd import fbgmm, unigram_acoustic_wordseg as uaw
from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
from segmentalist_amd.synth import make_corpus
from tests.golden import cases

which = sys.argv[1]
fb_type = sys.argv[2] if len(sys.argv) > 2 else "standard"      # viterbi: k_fbb_segment<BAND, true> / k_fbb_slots<.., true>
D, K, W, U = 8, 10, 6, 2000
t0 = time.time()
if which == "ragged":
    corpus = make_corpus(U, D, K, seed=110, ragged=True, n_slices_max=W, N_range=(3, 150))
else:
    corpus = make_corpus(U, D, K, seed=110, N=150 if which == "n150" else 64, n_slices_max=W)
random.seed(5); np.random.seed(5)
seg = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, FixedVarPrior(*cases.fixed_prior_params(D)), *corpus, covariance_type="fixed",
                                 fb_type=fb_type, n_slices_min=0, n_slices_max=W, p_boundary_init=0.5, beta_sent_boundary=-1,
                                 lms=1.0, wip=0.0, init_am_assignments="rand", time_power_term=1.0, sync="batch",
                                 n_gibbs_blocks=8, n_stat_blocks=8, batch_seed=11, score_precision="f64")
print(which, "built in %.1f s, N_max %d" % (time.time() - t0, seg._corpus.N_max), flush=True)
for sw in range(4):
    seg.batch_sweep_async()
torch.cuda.synchronize()
seg._df.check_status()
t1 = time.time()
for sw in range(6):
    seg.batch_sweep_async()
torch.cuda.synchronize()
print(which, "6 sweeps: %.3f ms per sweep" % (1e3 * (time.time() - t1) / 6), flush=True)
