"""Every `VLMC_*` environment variable this build reads, in ONE place, each with its default next to its description.

Three kinds, and only the first is an interface:

PUBLIC (ten): what a user of the drop-in pruners may want to set.  Everything works with none of them set.

CROSSCHECK: the alternative routes that exist so that the tests can hold every kernel / engine route against the one it replaced, on
the GPU, inside whole prunes (`VLMC_CROSSCHECK=name[,name..]` names them: vlmc/crosscheck.py).  Not a second backend: nothing in the
product selects them, and a route that was measured and lost is deleted, not parked here (round 6 removed the GEMM epilogue folds,
the padding length buckets and the SparseGPT look-ahead).

INTERNAL: measurement aids of bench.py / tools/, tuning overrides of single kernels, test hooks.

Each entry is `name: (default, description)`; the default is the string an unset variable reads as (None: no value).  The package
reads them through `flag`, `integer` and `text` below, the library through `env_flag` / `env_int` / `env_text` (csrc/common.hpp),
and both follow ONE rule: a flag is on unless its value is "0".  vlmc/crosscheck.py is the one writer.

`tests/test_abi.py::test_every_environment_switch_is_registered_with_its_default` greps the tree: a `VLMC_*` variable that is read anywhere but not
listed here, or read other than through those readers, fails the build's CPU tests."""
from __future__ import annotations

import os

PUBLIC = {
    "VLMC_LIB": (None, "path of another build of libvlmc_hip.so (default: the in-tree one next to this package)"),
    "VLMC_FAST": ("1", "0: every launch through ctypes instead of the compiled host path vlmc/_fast (same C ABI, same kernels)"),
    "VLMC_BATCH_REPLAY": ("128", "calibration samples per block forward of the replay (128 = all; 1 = the reference's per-sample loop)"),
    "VLMC_REPLAY_TOKENS": ("65536", "activation rows per block forward at most"),
    "VLMC_SHARD_CALIB": ("1", "0: under torch.distributed every rank is a replica that sees all samples (the reference's behaviour); default: samples sharded, statistics all-gathered"),
    "VLMC_RELEASE_MEMORY": ("0", "1: free cached device memory after every tower (the reference's `torch.cuda.empty_cache()` habit; costs time)"),
    "VLMC_CROSSCHECK": ("", "comma-separated names of cross-check routes (vlmc/crosscheck.py), or `all`"),
    "VLMC_STRICT": ("0", "1: an exception inside an optional fast path (the stacked capture) is raised instead of falling back to the reference's route"),
    "VLMC_VERBOSE": ("0", "1: the pruners print what the reference prints per linear"),
    "VLMC_PHASE_TIMERS": ("0", "1: synchronising per-phase timers (vlmc/phases.py; bench.py's sub-totals)"),
}

# every variable vlmc/crosscheck.py's ROUTES set (kept in step by the test); "the default route" is the one the product runs
CROSSCHECK = {
    "VLMC_GEMM_RING": ("1", "0: the register-staged GEMM kernel for every shape"),
    "VLMC_GEMM_PINGPONG": ("1", "0: both waves of a SIMD in lockstep"),
    "VLMC_GEMM_WIDE": ("1", "0: K-steps of 32 with half-line requests for every K"),
    "VLMC_GEMM_PERSIST": ("1", "0: one GEMM workgroup per tile"),
    "VLMC_GEMM_EDGE": ("1", "0: half panels / blocks are scheduled like full ones"),
    "VLMC_GEMM_SMALL_TILES": ("1", "0: 128 x 128 tiles also where a launch makes few workgroups of them"),
    "VLMC_GEMM_WIDE_SLOTS": ("0", "2: the shallow ring also for the tiles of at most 64 x 64"),
    "VLMC_LINEAR_GROUP": ("1", "0: every linear its own launch"),
    "VLMC_LINEAR_FWD": ("1", "0: the GEMM library for the blocks' linears"),
    "VLMC_LINEAR_F32": ("1", "0: fp32 modules left to the GEMM library"),
    "VLMC_MATRIX_FUSED": ("1", "0: the multi-launch matrix-wide select"),
    "VLMC_SELECT_MIXED": ("1", "0: one row-select launch per width"),
    "VLMC_DSNOT_RADIX_ONLY": ("0", "1: DSnoT list heads by the exact radix route only"),
    "VLMC_DSNOT_LISTS": ("1", "0: DSnoT by the per-cycle arg-min kernel"),
    "VLMC_TOWER_BATCH": ("1", "0: finished towers run per sample"),
    "VLMC_GRAPH_REPLAY": ("1", "0: no HIP graphs anywhere in the replay"),
    "VLMC_SKIP_DEAD_TAIL": ("1", "0: the statistics pass runs every block to its end"),
    "VLMC_LATER_EQUAL": ("1", "0: remembered tower inputs compared at once"),
    "VLMC_TOWER_BATCHED_TRACE": ("1", "0: the forward that traces a finished tower's wiring runs the tower for its one sample"),
    "VLMC_TOWER_TRACES": ("1", "identical traces before a finished tower's wiring is used"),
    "VLMC_TOWER_PREDICT": ("1", "0: finished towers learn every sample's block-0 arguments from an aborted forward"),
    "VLMC_TOWER_MEMO": ("1", "0: finished towers are run again in every capture phase"),
    "VLMC_TOWER_GRAPH": ("1", "0: finished towers are not replayed from HIP graphs"),
    "VLMC_SGPT_CONCURRENT": ("1", "0: one SparseGPT Hessian at a time"),
    "VLMC_SGPT_STACK": ("1", "0: one SparseGPT linear at a time"),
    "VLMC_SGPT_SELECT_SWEEP": ("1", "0: the block threshold by the multi-launch radix select, sweep with the mask handed in"),
    "VLMC_SGPT_SYRK": ("1", "0: library GEMM Hessian"),
    "VLMC_SGPT_DIRECT_FACTOR": ("1", "0: the reference's three-step factor chain"),
    "VLMC_CHOL_GRAPH": ("1", "0: the blocked Cholesky issued launch by launch instead of from a HIP graph"),
    "VLMC_SGPT_DEFER": ("1", "0: one Hessian update per hook call"),
    "VLMC_SGPT_PERSISTENT": ("1", "0: the factorization as a chain of launches per 128 columns"),
    "VLMC_RMS_NORM": ("1", "0: the language-model blocks' RMS norms run as the model files' seven launches"),
    "VLMC_SDPA_DMA": ("1", "0: K and V of vlmc_sdpa staged through registers"),
    "VLMC_SDPA": ("1", "0: F.scaled_dot_product_attention inside a replayed block left to torch"),
    "VLMC_ATTN_DMA": ("1", "0: K / V of vlmc_attn_fwd staged through registers"),
    "VLMC_ATTN_MATMUL": ("1", "0: the blocks' batched matmuls left to torch during the replay"),
    "VLMC_ROW_MEAN": ("1", "0: the norms' fp32 mean left to torch during the replay"),
    "VLMC_ATTN_TR": ("1", "0: attn @ v with the operand transposed while writing LDS"),
    "VLMC_LORA_FUSED": ("1", "0: SparseLoRA through a materialised W_eff and library GEMMs"),
    "VLMC_GELU": ("1", "0: torch's GELU kernel during the replay"),
    "VLMC_GELU_MUL": ("1", "0: a gated FFN's gelu(wi_0(h)) * wi_1(h) runs as vlmc_gelu plus torch's mul over every row"),
    "VLMC_ATTN_FUSED": ("1", "0: an attention written op by op runs op by op"),
    "VLMC_ATTN_PRE": ("1", "0: the qkv bias add and the q scale of an EVA attention run as torch's passes in front of vlmc_attn_fwd"),
    "VLMC_PAD_RAGGED": ("1", "0: ragged samples forwarded in groups of equal shape, never padded"),
    "VLMC_TOWER_PAD": ("1", "0: a finished tower runs one stacked pass per token count"),
    "VLMC_TOWER_SHARE_WIRING": ("1", "0: a finished tower is traced once per exact argument signature"),
    "VLMC_SGPT_BLOCK_LOOP": ("1", "0: the SparseGPT block loop issued from Python, launch by launch"),
    "VLMC_ROW_MAP": ("1", "0: the linears of a padded forward compute every row"),
    "VLMC_CAPTURE_MERGED": ("1", "0: one forward per calibration batch in the capture phases"),
    "VLMC_CAPTURE_MERGED_RAGGED": ("1", "0: ragged batches are captured one forward per sample"),
    "VLMC_SOFTMAX": ("1", "0: torch's softmax during the replay"),
    "VLMC_CAPTURE_MERGED_PRUNED": ("1", "0: ragged batches with a pruned tower on the way are captured one forward per sample"),
    "VLMC_ROW_SLICES": ("1", "0: a token slice of a padded fp32 stack is multiplied with its padding rows"),
    "VLMC_MEMO_COPY": ("0", "1: what a finished tower remembers of a capture phase is copied instead of kept with its version"),
    "VLMC_TORCH_FUNCTION_MODE": ("0", "1: the replay's routing through a scoped TorchFunctionMode instead of attribute patches"),
    "VLMC_ATTN_CLAMP": ("1", "0: an attention chain with the LLaMA clamp (torch.max against finfo.min) is computed op by op from the clamp on"),
    "VLMC_ROPE": ("1", "0: apply_rotary_pos_emb of a LLaMA attention runs as the model file's ~16 launches"),
    "VLMC_DSNOT_PAD": ("1", "0: the DSnoT pruners forward ragged samples in groups of equal shape (their statistic without per-sample token counts)"),
    "VLMC_SGPT_PAD": ("0", "1: the SparseGPT pruners forward ragged samples as one padded group per block pass, their Hessians over the group's row map (off: its gain over the groups of equal shape was within the measurement's spread, profiles/ragged_dsnot_sparsegpt.md)"),
    "VLMC_GROUP_VIEWS": ("1", "0: a merged forward's group is handed copies of a finished tower's block outputs, not views"),
}

INTERNAL = {
    # measurement aids
    "VLMC_SIMULATE_WORLD": ("0", "bench.py --calib-local: one process rehearses rank 0 of W (warns: the masks are not a real prune's)"),
    "VLMC_BENCH_ONE_DEVICE": ("0", "bench.py: rehearse the N > 1 code path with every rank on cuda:0 over gloo"),
    "VLMC_DEBUG_TOWERS": ("0", "1: print what every finished tower decides per calibration forward"),
    "VLMC_GC_FREEZE": ("1", "0: do not freeze the garbage collector's old generation for the duration of a prune"),
    "VLMC_CAPTURE_STREAMS": ("4", "side streams of the per-sample capture route"),
    "VLMC_CAPTURE_MERGED_MIN": ("24", "fewest calibration batches per rank for the stacked capture"),
    # tuning overrides of single kernels / routes (A/B runs of tools/)
    "VLMC_GEMM_BIG_TILES": ("200", "tiles needed to pick 256 x 256 (0 = never)"),
    "VLMC_GEMM_SHAPE": (None, "128 / 64 / p32 / 32: one small tile shape for every launch below the 256 x 256 threshold"),
    "VLMC_DSNOT_NW": ("0", "waves per workgroup of the DSnoT kernels (0: the size rule)"),
    "VLMC_SQNORM_VEC": ("0", "vector width of act_sqnorm (0: the size rule)"),
    "VLMC_F32_TILE": ("0", "128 / 64 / 32: one tile size for every fp32 GEMM launch (same bits)"),
    "VLMC_LORA_BQ": ("0", "192 / 256: activation rows per generated W_eff tile"), "VLMC_LORA_DBG": ("0", "lora_gemm ablation bits (results invalid)"),
    "VLMC_LORA_RECOMPUTE": ("0", "1: regenerate W_eff in the unfused backward instead of keeping it"),
    "VLMC_SGPT_SWEEP_STREAMS": ("4", "streams for the sweeps of a block's independent linears"),
    "VLMC_SGPT_SHARD_LAYERS": ("1", "0: under torch.distributed every rank prunes every linear"),
    "VLMC_SGPT_SYRK_F32": ("0", "1: fp32 activations take the nine-plane SYRK"),
    "VLMC_SGPT_SORT_THRESHOLD": ("0", "1: the block threshold by torch.sort (the reference's op)"),
    "VLMC_SGPT_PERSISTENT_WGS": ("128", "workgroups of the persistent factorization"),
    "VLMC_SGPT_INVERSE_FORK": ("0", "1: the inverse's rows on a second stream inside the graph (measured slower)"),
    "VLMC_CHOL_PANEL_GEMM": ("1", "0: library triangular solve for the panel"),
    # test hooks
    "VLMC_SGPT_SELECT_FORCE_FAIL": ("0", "tests: make the one-launch sweep's grid barrier fail at a given level"),
    "VLMC_MATRIX_FORCE_SLOW": ("0", "tests: make the fused matrix-wide select take its slow route at a given barrier"),
    "VLMC_MATRIX_FUSED_WGS": (None, "tests: workgroups of the fused matrix-wide select at most (default: the device's CU count)"),
}

DEFAULTS = {name: default for table in (PUBLIC, CROSSCHECK, INTERNAL) for name, (default, _doc) in table.items()}


def all_names():
    return set(DEFAULTS)


def _unregistered(name):
    return KeyError(f"{name} is not registered in vlmc/config.py")


def flag(name):
    """On unless the variable's value (or its default) is "0"."""
    try:
        return os.environ.get(name, DEFAULTS[name]) != "0"
    except KeyError:
        raise _unregistered(name) from None


def integer(name):
    """int() of the variable's value (or its default); a value that is not an integer raises ValueError."""
    try:
        return int(os.environ.get(name, DEFAULTS[name]))
    except KeyError:
        raise _unregistered(name) from None


def text(name):
    """The variable's value, or its default (which may be None)."""
    try:
        return os.environ.get(name, DEFAULTS[name])
    except KeyError:
        raise _unregistered(name) from None
