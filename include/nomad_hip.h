/*
 * nomad_hip.h - C ABI of libnomad_hip.so, the MI355X (gfx950) NOMAD scoring engine.
 *
 * The reference (alessandroragano/nomad) has no FFI boundary of its own: its hot path is Python
 * calling into fairseq/PyTorch/SciPy.  Each entry point below replaces one such call site
 * (paths relative to /root/reference):
 *
 *   nomad_create / nomad_destroy   Nomad.__init__ model construction + load_state_dict
 *                                  (src/nomad_audio/nomad.py:57-71)
 *   nomad_embed                    TripletModel.forward (nomad.py:224-231) and
 *                                  LossNetLayers.forward (nomad.py:243-258): wav2vec 2.0 BASE
 *                                  backbone (fairseq Wav2Vec2Model, call sites nomad.py:226,245)
 *                                  + mean/ReLU/Linear/L2-normalise head
 *   nomad_pairwise                 scipy cdist + np.mean(axis=1) (nomad.py:108-111)
 *   nomad_embed_features[_ragged]  Origw2v.forward (src/models/networks.py:29-34): the backbone's output averaged over time,
 *                                  the raw wav2vec 2.0 baseline of the evaluation experiments (eval_w2v: True)
 *   nomad_cdist                    cdist + np.mean(axis=1) of src/training/train_triplet.py (:281-282, :327-328, :385-386)
 *                                  on rows of any width (768 for the baseline)
 *   nomad_paired_distance          np.diag(cdist(test, ref)) (train_triplet.py:438-439) without the matrix
 *   nomad_cdist_backward           d / d a and d / d b of nomad_cdist's matrix and row means (the NOMAD score as a loss)
 *   nomad_knn / nomad_knn_backward the k nearest rows of a bank and their mean distance, matrix-free, and its gradient (the
 *                                  nearest-reference NOMAD score as a score and as a loss)
 *   nomad_embed_windows_backward   d / d waveform of the window embeddings (scores over time as a loss)
 *   nomad_degrade_noise / _clip    noise at a target SNR and percentile clipping of src/utils/degradations.py (:30-68, :70-83), G levels
 *                                  per clip, written as the packed batch nomad_embed_ragged reads
 *   nomad_degrade_convolve         every clip convolved with G impulse responses (reverberation as a causal FIR filter), same layout
 *   nomad_degrade_reverb           sox's `reverb P` of src/utils/degradations.py (:97-101) as comb and all-pass recurrences, G reverberance
 *                                  levels per clip, same layout (restated from memory of sox 14.4; not checked against the binary)
 *   nomad_degrade_normalize        BS.1770-4 loudness (or rms / peak level) of packed rows and the linear gain to a target, in place:
 *                                  the ffmpeg-normalize step of audio_degrader_training.py / audio_degrader_test.py
 *   nomad_gammatone / nomad_nsim   gammatone spectrograms of packed rows and the NSIM of each degraded row with its clean clip: the
 *                                  similarity src/utils/nsim_triplet_sampling.py samples triplets from (modelled on ViSQOL's speech mode
 *                                  from memory; not checked against the binary)
 *   nomad_nsim_patches             the same similarity patch by patch: the clean clip's active patches, each searched for in the
 *                                  degraded spectrogram, so that a delay may change inside a file and silence does not count
 *   nomad_align_delay / _shift     the delay of every degraded row against its clean clip (the largest cross-correlation over integer
 *                                  lags) and the rows moved by it: what files with codec delay need ahead of nomad_nsim
 *   nomad_wav_probe / _read_rows   torchaudio.load + channel mean + Resample of load_processing (nomad.py:196-205)
 *   nomad_l1_loss                  NomadLoss.forward (nomad.py:267-282)
 *
 * Conventions: every function returns 0 on success or a negative nomad_status; nothing throws.
 * All `dev` pointers are device (HBM) pointers owned by the caller; `host` pointers are host
 * memory.  Compute entry points are asynchronous on the caller's hipStream_t and never allocate:
 * scratch comes from the caller-provided workspace (size from nomad_workspace_bytes).  A context
 * is bound to one device and is not re-entrant.  The library has no CPU fallback: without a
 * gfx950 device nomad_create fails with NOMAD_ERR_NO_DEVICE.
 *
 * Calling contract (what every entry point that takes a nomad_stream_t keeps; tests/test_gpu_stream_order.py and the
 * unaligned cases of tests/test_gpu_degrade.py, test_gpu_convolve.py and test_gpu_loudness.py hold the library to it):
 *   Stream.  ALL device work of a call - kernels, memsets, the copy of its host arrays - is queued on the stream the caller
 *     passes, in order: it reads its inputs behind whatever the caller queued there before, and whatever the caller queues there
 *     afterwards sees its outputs.  Nothing is launched on the legacy default stream or on a stream of the library's own; the only
 *     exceptions are one-time preparation (nomad_create, nomad_enable_*, nomad_train_enable), which synchronises the device
 *     before it returns.  (nomad_amd.Engine's two-stream batch split is host-layer code: it joins its side stream to the
 *     caller's stream on both sides of the call.)
 *   Host arrays.  Every `*_host` array - lengths, levels and SNRs, response lengths, span tables, loss weights and frame counts -
 *     is consumed before the call returns: the caller may overwrite or free it at once, while the stream still has the call's
 *     work ahead of it.  The library keeps its own copy in one of three rings of 16 slots per context (ragged metadata and span
 *     tables; weighted-loss metadata; degradation metadata) until the asynchronous copy has run, so at most 16 such calls of
 *     one family may be queued on a context without the stream having caught up (a span call takes two slots); the 17th
 *     reuses the first one's slot.
 *   Alignment.  Device pointers are expected 16-byte aligned: what hipMalloc and torch's allocator return, and any slice of
 *     whole rows of such a buffer whose row is a multiple of 16 bytes (packed ragged rows: stride % 4 == 0; embeddings; layer
 *     outputs).  Two exceptions need only the 4-byte alignment of a float: a [B][n_samples] waveform batch may be passed
 *     from any whole row on, whatever n_samples is (the front end reads samples one by one); and the sample rows of the five
 *     degradation calls - x_dev, out_dev, noise_dev and ir_dev of nomad_degrade_noise / _clip / _convolve / _reverb / _normalize - which
 *     are read and written sample by sample (convolve and normalize move 16 bytes at a time only where they find the addresses
 *     aligned).  Workspaces, scratch and float64 statistics are always 16-byte aligned.
 */
#ifndef NOMAD_HIP_H
#define NOMAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NOMAD_NUM_LAYERS 12
#define NOMAD_EMBED_DIM 768
#define NOMAD_EMB_DIM 256

typedef enum nomad_status {
    NOMAD_OK = 0,
    NOMAD_ERR_INVALID = -1,   /* bad argument */
    NOMAD_ERR_NO_DEVICE = -2, /* no usable gfx950 device */
    NOMAD_ERR_HIP = -3,       /* a HIP runtime call failed; see nomad_last_error() */
    NOMAD_ERR_WORKSPACE = -4, /* workspace too small */
    NOMAD_ERR_IO = -5,        /* a file could not be opened / read (nomad_wav_*) */
    NOMAD_ERR_FORMAT = -6     /* not a RIFF/WAVE file, or an encoding nomad_wav_read_rows does not decode */
} nomad_status;

typedef struct nomad_ctx nomad_ctx;
typedef void* nomad_stream_t; /* hipStream_t */

/* One transformer encoder layer, fairseq TransformerSentenceEncoderLayer parameter names.
 * All matrices are row-major [out][in] exactly as torch.nn.Linear stores them. */
typedef struct nomad_layer_weights {
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b; /* self_attn.{q,k,v,out}_proj */
    const float *ln1_w, *ln1_b;                                 /* self_attn_layer_norm */
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;                 /* fc1 [3072][768], fc2 [768][3072] */
    const float *ln2_w, *ln2_b;                                 /* final_layer_norm */
} nomad_layer_weights;

/* HOST pointers, fp32, in the layout of the reference checkpoint nomad_best_model.pt
 * (keys ssl_model.* / embedding_layer.1.*; nomad.py:63-65).  nomad_create copies and repacks
 * them; the caller may free them afterwards. */
typedef struct nomad_weights {
    const float* conv_w[7];          /* feature_extractor.conv_layers.i.0.weight: [512][1][10], 4x[512][512][3], 2x[512][512][2] */
    const float *gn_w, *gn_b;        /* feature_extractor.conv_layers.0.2 (GroupNorm 512) */
    const float *feat_ln_w, *feat_ln_b; /* layer_norm (512) */
    const float *proj_w, *proj_b;    /* post_extract_proj [768][512] */
    const float *pos_v, *pos_g, *pos_b; /* encoder.pos_conv.0 weight_v [768][48][128], weight_g [128], bias */
    const float *enc_ln_w, *enc_ln_b;   /* encoder.layer_norm */
    nomad_layer_weights layers[NOMAD_NUM_LAYERS];
    const float *emb_w, *emb_b;      /* embedding_layer.1 [256][768], [256] */
} nomad_weights;

/* ---- lifetime ---------------------------------------------------------------------------- */
int nomad_create(nomad_ctx** out, int device, const nomad_weights* host_weights);
void nomad_destroy(nomad_ctx* ctx);
const char* nomad_last_error(void);
const char* nomad_version(void);
/* Binary-interface number of this header.  It changes whenever an entry point's signature or a struct layout changes in a way an
 * already compiled caller would not survive; a caller compares nomad_abi_version() of the library it loaded with the
 * NOMAD_ABI_VERSION it was compiled against BEFORE any other call (nomad_amd/_lib.py does).  History: 2 -> 3 (round 5/6):
 * nomad_set_concurrent_parts(int) became nomad_set_concurrent_parts(nomad_ctx*, int) - a caller built against the old header
 * would pass its int where the context pointer goes. */
#define NOMAD_ABI_VERSION 3
int nomad_abi_version(void);
/* How this library was built, as a bit set.  NOMAD_BUILD_PACKED_FP32: the device code may contain packed-FP32 VALU
 * instructions (v_pk_fma_f32 ...), which on gfx950 can lose a product while a bf16 MFMA kernel of ANOTHER stream shares the
 * SIMD (DESIGN.md "The packed-FP32 hazard") - the shipped build has none, and a host layer must not co-schedule two forwards
 * of a context on two streams when this bit is set (nomad_amd.Engine switches its two-stream batch split off).  The library's
 * own 128 x 128 bf16 GEMM can still disturb third-party kernels that use packed FP32 on other streams.
 * NOMAD_BUILD_DIAG: libnomad_diag.so (every experimental instantiation and probe). */
#define NOMAD_BUILD_PACKED_FP32 1
#define NOMAD_BUILD_DIAG 2
int nomad_build_flags(void);
/* Scheduling hint: into how many parts, on as many streams, the host layer splits the batches it submits CONCURRENTLY (1 = one
 * forward at a time, the default).  Results never depend on it - every fp32 GEMM instantiation contracts k in the same order -
 * only the tile-shape choice does: next to another stream's kernels the 128 x 128 tiles' extra operand traffic costs more
 * (measured: the 256 x 128 / 128 x 128 price ratio that minimises the bench step is 1.08 with two concurrent halves, 1.03 with
 * one forward).  nomad_amd.Engine calls it with its split count.  Per context (round 5: it was process-wide state); like every
 * other call on a context it must not race with another host thread's call on the SAME context.  The library keeps no mutable
 * process-wide state that affects results (what is process-wide: the last-error text, the once-per-kernel LDS-attribute flags, the
 * diagnostic library's timeline buffer) and never reads the environment (tests/test_abi.py holds libnomad_hip.so to "imports no getenv").
 * Returns 0, or NOMAD_ERR_INVALID for a null context or parts < 1. */
int nomad_set_concurrent_parts(nomad_ctx* ctx, int parts);

/* ---- shapes ------------------------------------------------------------------------------ */
/* Encoder frames T for a clip of n_samples (conv stack (10,5),(3,2)x4,(2,2)x2); <=0 if too short. */
int nomad_num_frames(int n_samples);
/* Scratch bytes nomad_embed needs for a (B, n_samples) batch. */
int nomad_workspace_bytes(const nomad_ctx* ctx, int B, int n_samples, size_t* bytes);

/* ---- hot path ---------------------------------------------------------------------------- */
/*
 * Embed B clips of n_samples each.
 *   wav_dev     [B][n_samples] fp32 raw amplitude (nomad.py:225 squeezes (B,1,N) to this)
 *   head_w_dev/head_b_dev  optional override of the 768->256 head ([256][768],[256], device);
 *               NULL = the checkpoint's embedding_layer (TripletModel).  LossNetLayers has its own
 *               never-loaded embedding layer (nomad.py:238-241), which callers pass here.
 *   emb_dev     [B][256] fp32 unit-norm embeddings (out)
 *   layers_dev  optional [12][B][T][768] fp32 transformer layer outputs (out; nomad.py:248), or NULL
 */
int nomad_embed(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples,
                const float* head_w_dev, const float* head_b_dev,
                float* emb_dev, float* layers_dev,
                void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);

/*
 * Embed B clips of DIFFERENT lengths in one launch sequence, with no padding in the arithmetic (the
 * reference's per-file loop, nomad.py:171-183, batched): results are bit-identical to per-clip nomad_embed
 * calls.  wav_dev is [B][stride] fp32 with clip b occupying the first lengths_host[b] samples of its row
 * (the rest of the row is never read); lengths_host is a HOST array.
 */
int nomad_workspace_bytes_ragged(const nomad_ctx* ctx, int B, const int* lengths_host, size_t* bytes);
int nomad_embed_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                       const float* head_w_dev, const float* head_b_dev, float* emb_dev,
                       void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);

/*
 * Euclidean distance matrix + row means, computed in float64 in the difference form
 * sqrt(sum_k (a_k - b_k)^2) like scipy's cdist on float32 inputs promoted to double.
 *   deg_dev [Nd][256] fp32, ref_dev [Nr][256] fp32
 *   dist_dev  optional [Nd][Nr] float64 (out) or NULL;  mean_dev [Nd] float64 (out)
 * Scratch (row sums per 64-reference tile, 16 MB) is owned by the context, one block PER LAUNCH STREAM: calls on
 * different streams of one context may be in flight together; the first call on a stream the context has not seen
 * allocates that stream's block (the only entry point that may allocate after nomad_create).  That look-up is guarded by a
 * mutex in the context: host threads that each drive their own stream may call it concurrently.  (Every other entry point
 * that takes a context expects one driving host thread per context.)
 */
int nomad_pairwise(nomad_ctx* ctx, const float* deg_dev, int Nd, const float* ref_dev, int Nr,
                   double* dist_dev, double* mean_dev, nomad_stream_t stream);

/*
 * nomad_pairwise with the row width as an argument: a_dev [Na][D], b_dev [Nb][D] fp32, D a positive multiple of 4, at most 4096.
 * Arithmetic contract (both functions): per pair ONE float64 accumulator, e = (double)a_k - (double)b_k, acc = fma(e, e, acc), k
 * ascending from 0, then sqrt(acc); row sums per 64-column tile in column order, tiles added in order.  At D = 256 nomad_cdist
 * returns the bits of nomad_pairwise.  Scratch: the context's per-stream block of nomad_pairwise, under the same rules.
 *   dist_dev  optional [Na][Nb] float64 (out) or NULL;  mean_dev [Na] float64 (out)
 * NOMAD_ERR_INVALID: a NULL operand or mean_dev, Na / Nb <= 0, D not a multiple of 4 or outside 4 .. 4096.
 */
int nomad_cdist(nomad_ctx* ctx, const float* a_dev, int Na, const float* b_dev, int Nb, int D,
                double* dist_dev, double* mean_dev, nomad_stream_t stream);
/* out_dev[i] = ||a_i - b_i|| for i < N, [N] float64: bit-identical to the diagonal of nomad_cdist(a, N, b, N, D), without the
 * other N - 1 columns.  No scratch, no allocation.  NOMAD_ERR_INVALID as for nomad_cdist. */
int nomad_paired_distance(nomad_ctx* ctx, const float* a_dev, const float* b_dev, int N, int D,
                          double* out_dev, nomad_stream_t stream);

/*
 * The backward of nomad_cdist: gradients of  sum_ij gdist_ij d_ij + sum_i gmean_i mean_i  with respect to a and b.
 * Let d_ij be the value nomad_cdist computes (the same chain, the same bits) and c_ij = gdist_ij + gmean_i / Nb, formed in
 * float64, a NULL upstream counting as 0.  Then
 *   W_ij  = c_ij / d_ij, and exactly 0 where d_ij == 0 (torch.cdist's convention: a row of b equal to the row of a contributes
 *           nothing, never NaN / Inf)
 *   da_ik = (float) sum_j fma(W_ij, (double)a_ik - (double)b_jk, acc),  j ascending from 0, one float64 accumulator
 *   db_jk = (float) sum_i fma(W_ij, (double)b_jk - (double)a_ik, acc),  i ascending from 0
 * each output rounded to fp32 once, at the store; no atomics, no partial sums whose number depends on the grid.  So results are
 * identical run to run, row i of da depends on a_i, b and row i of the upstreams only (the bits of the row's own Na = 1 call), and
 * row j of db on b_j, a and column j of gdist (and gmean) only (the bits of its own Nb = 1 call with gmean / Nb folded into gdist).
 *   gdist_dev [Na][Nb] float64 or NULL, gmean_dev [Na] float64 or NULL (not both NULL)
 *   da_dev [Na][D] fp32 (out) or NULL, db_dev [Nb][D] fp32 (out) or NULL (not both NULL)
 * Scratch is the caller's: nomad_cdist_backward_scratch_bytes(Na, Nb) bytes (the [Na][Nb] float64 W), written before it is read.
 * Asynchronous, no allocation; argument errors return before anything is queued.
 * NOMAD_ERR_INVALID: NULL a / b / scratch, both upstreams NULL, both outputs NULL, Na / Nb <= 0 (or above 65535 * 64), D not a
 * multiple of 4 or outside 4 .. 4096.  NOMAD_ERR_WORKSPACE: scratch_bytes too small.
 */
int nomad_cdist_backward_scratch_bytes(int Na, int Nb, size_t* bytes);
int nomad_cdist_backward(nomad_ctx* ctx, const float* a_dev, int Na, const float* b_dev, int Nb, int D,
                         const double* gdist_dev, const double* gmean_dev, float* da_dev, float* db_dev,
                         void* scratch_dev, size_t scratch_bytes, nomad_stream_t stream);

/*
 * Nearest references: per row of a the k rows of b at the smallest distance, and their mean - the NOMAD score against the closest
 * part of a mixed bank - without forming the [Na][Nb] matrix.  a_dev [Na][D], b_dev [Nb][D] fp32 as for nomad_cdist, 1 <= k <= 64,
 * k <= Nb.  Contract (held bit for bit by tests/test_gpu_knn.py):
 *   d_ij          the value nomad_cdist computes: the same chain, the same bits (at D = 256 those of nomad_pairwise).  With
 *                 dist_dev given, that [Na][Nb] float64 matrix is nomad_cdist's; NULL: it is never formed.
 *   neighbours    of row i: the k columns smallest under the key (d_ij, j), ascending; a NaN distance is ordered as +infinity,
 *                 equal keys by index.  So equal distances resolve to the lower index, every output slot is always written and
 *                 every index lies in 0 .. Nb - 1, whatever the input.  (The kernels pad a last 64-column tile with copies of the
 *                 last row of b; those are excluded by index, not by value.)
 *   knn_dist_dev  [Na][k] float64 (out): the r-th neighbour's d, as stored in the matrix (NaN stays NaN);
 *   knn_idx_dev   [Na][k] int32 (out): its column.  With k = Nb the index row is the stable argsort of the matrix row.
 *   score_dev     [Na] float64 (out): (sum_{r=0}^{k-1} knn_dist[i][r], r ascending, one float64 accumulator from 0.0) / (double)k.
 * Row i of every output depends on a_i and b only: its bits are those of its own Na = 1 call, the same with and without dist_dev
 * and the same run to run; no atomics.  Scratch is the caller's: nomad_knn_scratch_bytes(Na, Nb, k) bytes (the k best of every
 * 64-column tile, 12 bytes each), written before it is read.  Asynchronous, no allocation; argument errors return before
 * anything is queued.  Time is accounted to the distance stage's profile class.
 * NOMAD_ERR_INVALID: a NULL operand, output (other than dist_dev) or scratch, Na / Nb <= 0 or above 65535 * 64, D not a multiple
 * of 4 or outside 4 .. 4096, k < 1, k > 64 or k > Nb.  NOMAD_ERR_WORKSPACE: scratch_bytes too small.
 */
int nomad_knn_scratch_bytes(int Na, int Nb, int k, size_t* bytes);
int nomad_knn(nomad_ctx* ctx, const float* a_dev, int Na, const float* b_dev, int Nb, int D, int k,
              double* dist_dev, double* knn_dist_dev, int* knn_idx_dev, double* score_dev,
              void* scratch_dev, size_t scratch_bytes, nomad_stream_t stream);

/*
 * The backward of nomad_knn: gradients of  sum_ir g_knn_ir knn_dist_ir + sum_i g_score_i score_i  with respect to a and b, the
 * selection held fixed.  With c_ir = g_knn_ir + g_score_i / k (float64, a NULL upstream counting as 0) the outputs are BY DEFINITION
 * the bits of nomad_cdist_backward called with gmean_dev = NULL and the dense gdist_ij = c_ir where j = knn_idx[i][r], 0 elsewhere:
 * its order of summation, its single rounding, its rows' independence of the grid; a neighbour at distance 0 contributes nothing and
 * is never NaN / Inf; one output alone has the bits it has next to the other.
 *   knn_idx_dev [Na][k] int32, as nomad_knn wrote it (distinct within a row); an index outside 0 .. Nb - 1 is skipped
 *   g_knn_dev [Na][k] float64 or NULL, g_score_dev [Na] float64 or NULL (not both NULL)
 *   da_dev [Na][D] fp32 (out) or NULL, db_dev [Nb][D] fp32 (out) or NULL (not both NULL)
 * Scratch is the caller's: nomad_knn_backward_scratch_bytes(Na, Nb, k) bytes (that dense upstream and nomad_cdist_backward's W, two
 * [Na][Nb] float64 matrices), written before it is read.  Asynchronous, no allocation; argument errors return before anything is
 * queued.  NOMAD_ERR_INVALID: as for nomad_knn, or both upstreams NULL, or both outputs NULL.  NOMAD_ERR_WORKSPACE: scratch_bytes
 * too small.
 */
int nomad_knn_backward_scratch_bytes(int Na, int Nb, int k, size_t* bytes);
int nomad_knn_backward(nomad_ctx* ctx, const float* a_dev, int Na, const float* b_dev, int Nb, int D, int k,
                       const int* knn_idx_dev, const double* g_knn_dev, const double* g_score_dev,
                       float* da_dev, float* db_dev, void* scratch_dev, size_t scratch_bytes, nomad_stream_t stream);

/*
 * Pooled backbone features, Origw2v.forward (networks.py:29-34): the last encoder layer's output averaged over time - no
 * ReLU, no Linear, no normalisation, no embedding.  feat_dev [B][768] fp32 (out).  `precision` selects the forward: the one of
 * nomad_embed / nomad_embed_bf16x3 / nomad_embed_bf16 (and their ragged forms), with that entry point's preconditions
 * (nomad_enable_bf16x3 / nomad_enable_bf16 first), its workspace size (nomad_workspace_bytes* of that precision and geometry)
 * and its statuses for bad arguments; an unknown precision is NOMAD_ERR_INVALID.  Asynchronous, no allocation,
 * deterministic; a clip's 768 values do not depend on the batch it is in: the ragged call is bit-identical to one uniform
 * call per clip.
 */
enum { NOMAD_PRECISION_F32 = 0, NOMAD_PRECISION_BF16X3 = 1, NOMAD_PRECISION_BF16 = 2 };
int nomad_embed_features(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, int precision,
                         float* feat_dev, void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
int nomad_embed_features_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                                int precision, float* feat_dev, void* workspace_dev, size_t workspace_bytes,
                                nomad_stream_t stream);

/*
 * Embeddings over windows of frames, from ONE forward: the head (time mean, ReLU, Linear(768, 256), L2 normalisation) applied
 * to windows of `win` encoder frames every `hop` frames instead of to the whole clip (one frame = 320 samples = 20 ms).
 * nomad_num_windows(T, win, hop): the windows of a clip of T >= 1 frames, win >= 1, hop >= 1: 1 if T <= win (one window over the
 * whole clip), else (T - win) / hop + 1; <= 0 for T, win or hop < 1.  Window k covers frames [k hop, k hop + min(win, T)); the
 * frames behind the last full window belong to no window (as with torch.Tensor.unfold).  Host arithmetic, no context.
 *   emb_dev  [sum_c W(T_c)][256] fp32 (out): clip 0's windows in order, then clip 1's, ... (B W(T) rows for equal lengths)
 * Each window's row is computed in the arithmetic of the plain head on the window's rows as if they were a clip of their own:
 * a window that covers a whole clip has the bits of that clip's embedding from nomad_embed* of the same precision, and a row
 * depends on its window's frames only (batch-invariant, deterministic, no atomics).  The encoder saw the whole clip: a window
 * is NOT the embedding of the excerpt alone.
 * `precision`, preconditions, workspace size and statuses are those of nomad_embed_features*.  The head override (both pointers
 * or neither) is for NOMAD_PRECISION_F32 only; with another precision, with win < 1 or hop < 1, or with a cut encoder
 * (nomad_set_encoder_depth) the call is NOMAD_ERR_INVALID.  Asynchronous, no allocation; argument errors return before anything
 * is queued.
 */
int nomad_num_windows(int T, int win, int hop);
int nomad_embed_windows(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, int precision, int win, int hop,
                        const float* head_w_dev, const float* head_b_dev, float* emb_dev,
                        void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
int nomad_embed_windows_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                               int precision, int win, int hop, const float* head_w_dev, const float* head_b_dev,
                               float* emb_dev, void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);

/*
 * NomadLoss: sum_{i<12} mean|a_layers[i]-b_layers[i]| + mean|a_emb-b_emb|.
 *   a_layers_dev/b_layers_dev [12][B][T][768]; a_emb_dev/b_emb_dev [B][256]; loss_dev [1] fp32 (out)
 *   scratch_dev: >= nomad_l1_scratch_bytes() bytes of device scratch.
 */
size_t nomad_l1_scratch_bytes(void);
int nomad_l1_loss(nomad_ctx* ctx, const float* a_layers_dev, const float* b_layers_dev,
                  const float* a_emb_dev, const float* b_emb_dev, int B, int T,
                  float* loss_dev, void* scratch_dev, nomad_stream_t stream);

/* ---- training: Nomad.forward() as a differentiable loss (nomad.py:142-146 + autograd) ------ */
/*
 * The reference back-propagates through the whole backbone to `estimate` (and, wastefully, into the
 * backbone parameters, which nobody uses: the freeze is commented out at nomad.py:74-76).  Here the
 * weights are frozen and only d loss / d waveform is computed.
 *
 *   nomad_enable_backward    builds the transposed weight copies once and a 32 MB split-K scratch (allocates; call
 *                            before training).  With it, nomad_embed_train / nomad_embed_backward cut the contraction
 *                            of their small-M GEMMs (fewer than 512 tiles of 64 x 64, e.g. 32 clips of 1 s) into 2 or 4
 *                            fixed slices summed in order - deterministic, but a different rounding than nomad_embed's,
 *                            whose summation order never depends on the batch.  Not in fine-tuning mode.
 *   nomad_embed_train        = nomad_embed with layers_dev mandatory; additionally fills `saved_dev`
 *                              (nomad_saved_bytes) with what the backward needs
 *   nomad_l1_loss_backward   d NomadLoss / d a_layers, d a_emb  (sign(a-b)/numel, times *upstream_dev)
 *   nomad_embed_backward     given d loss / d layers [12][B][T][768] (nullable) and d loss / d emb [B][256]
 *                            writes d loss / d wav [B][n_samples]; scratch: nomad_backward_workspace_bytes;
 *                            the gradient entering the conv feature extractor is scaled by feature_grad_mult (below)
 */
int nomad_enable_backward(nomad_ctx* ctx);
/*
 * fairseq's Wav2Vec2Model wraps the conv feature extractor's output in GradMultiply(features, feature_grad_mult)
 * whenever feature_grad_mult != 1 (wav2vec2.py, Wav2Vec2Model.forward; also in eval mode): the forward is the
 * identity, the gradient flowing back INTO the extractor - and so d loss / d waveform of Nomad.forward(),
 * nomad.py:142-146 - is multiplied by it.  The wav2vec 2.0 BASE config that wav2vec_small.pt carries (and that
 * load_model_ensemble_and_task keeps, nomad.py:58) has feature_grad_mult = 0.1, which is the default here;
 * 1.0 gives the plain chain rule, 0 means "extractor under no_grad" in fairseq and yields dwav = 0.
 * Applies to nomad_embed_backward only (the fine-tuning step never reaches the frozen extractor).
 */
int nomad_set_feature_grad_mult(nomad_ctx* ctx, float mult);
/*
 * Arithmetic of the fp32-layout GEMMs (nomad_embed, nomad_embed_ragged, nomad_embed_train, nomad_embed_backward,
 * nomad_train_backward): mode 0 (default) exact fp32 MFMA (v_mfma_f32_16x16x4_f32, the reference's arithmetic); mode 1
 * "bf16x3 products": every product a*w as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on the bf16 matrix cores, hi = bf16(x),
 * lo = bf16(x - hi) made in registers, fp32 accumulation - all buffers, epilogues and every other kernel unchanged.  A GEMM
 * is then within ~3e-5 (relative) of the fp32 one and its K loop ~5x shorter: for the small-M problems of Nomad.forward()
 * (nomad.py:142-146 at the shapes of nomad_loss_test.py:60-79) and of the fine-tuning step.  Opt-in: Nomad(precision=
 * "bf16x3").  The pos-conv and attention kernels stay fp32.
 */
int nomad_set_gemm_precision(nomad_ctx* ctx, int mode);
int nomad_get_gemm_precision(const nomad_ctx* ctx, int* mode);
int nomad_get_feature_grad_mult(const nomad_ctx* ctx, float* mult);
int nomad_saved_bytes(const nomad_ctx* ctx, int B, int n_samples, size_t* bytes);
int nomad_backward_workspace_bytes(const nomad_ctx* ctx, int B, int n_samples, size_t* bytes);
int nomad_embed_train(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples,
                      const float* head_w_dev, const float* head_b_dev, float* emb_dev, float* layers_dev,
                      void* saved_dev, size_t saved_bytes, void* workspace_dev, size_t workspace_bytes,
                      nomad_stream_t stream);
int nomad_l1_loss_backward(nomad_ctx* ctx, const float* a_layers_dev, const float* b_layers_dev,
                           const float* a_emb_dev, const float* b_emb_dev, int B, int T,
                           const float* upstream_dev, float* dlayers_dev, float* demb_dev, nomad_stream_t stream);
int nomad_embed_backward(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples,
                         const float* head_w_dev, const float* head_b_dev, const float* layers_dev,
                         const void* saved_dev, size_t saved_bytes, const float* dlayers_dev, const float* demb_dev,
                         float* dwav_dev, void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);

/* ---- exact-length (ragged) batches on the gradient paths ------------------------------------------------
 * The calls above over clips of DIFFERENT lengths, with no padding in the arithmetic - the layout of nomad_embed_ragged:
 * wav_dev / dwav_dev are [B][stride], clip b in the first lengths_host[b] samples of its row (the rest is never read);
 * every per-frame tensor is packed, M = sum_c T_c rows (T_c = nomad_num_frames(lengths_host[c])): layers_dev / dlayers_dev
 * are [12][M][768], emb / demb [B][256].  Sizes are functions of (B, lengths_host) and the context's switches only; the
 * forward's workspace is nomad_workspace_bytes_ragged.
 *
 *   nomad_embed_train_ragged     saved_dev == NULL (with saved_bytes == 0): the 12 layer outputs and the embedding, nothing kept,
 *                                no regularisation (the no-gradient branch of the loss; LossNetLayers over a ragged batch).
 *                                Else also fills saved_dev (nomad_saved_bytes_ragged) for the backward.
 *   nomad_embed_backward_ragged  dlayers_dev (nullable), demb_dev -> dwav_dev [B][stride]; the samples of a row behind its clip's
 *                                length are written as zero.  feature_grad_mult as in nomad_embed_backward.
 *   nomad_train_backward_ragged  accumulates into the context's gradient vector like nomad_train_backward.
 *   nomad_l1_loss_ragged / nomad_l1_loss_backward_ragged   (M, B) in place of (B, T): each layer term is the mean over the
 *                                M * 768 valid elements, the embedding term the mean over B * 256 - F.l1_loss on the
 *                                concatenation of the clips' valid frames.  With M = B * T the bits of the equal-length calls.
 *
 * Contract:
 *   - A clip's forward values (embedding, its rows of layers_dev, its saved activations) and its row of dwav_dev do not depend
 *     on the batch it is in: the ragged entry points NEVER split K, in fine-tuning mode or outside it (the equal-length loss
 *     path outside fine-tuning mode does, see nomad_enable_backward).  After nomad_train_enable they are the bits of the clip's
 *     own nomad_embed_train / nomad_embed_backward call at B = 1, and the embedding the bits of nomad_embed_ragged; an
 *     equal-length batch handed to the ragged entry points gives the bits of the equal-length entry points, the gradient
 *     vector included (same rows, same summation order).
 *   - nomad_train_set_stochastic / nomad_train_set_branches work as for equal lengths.  Mask element indices are those of the
 *     packed tensors: activation sites index [M][768] (dropout_input: row m of the packed post_extract_proj output),
 *     attention probabilities index clip c's [12][T_c][T_c] block at offset 12 * sum_{j<c} T_j^2 (64-bit) - an equal-length
 *     batch draws exactly the masks of the equal-length entry points.  Branches are equal groups of CLIPS (B % branches == 0),
 *     of any lengths.
 *   - Not supported, refused with NOMAD_ERR_INVALID: a trainable conv feature extractor (nomad_train_set_convnet(1); its dW
 *     operands are laid out per clip in equal column blocks) together with a ragged call.  nomad_train_set_frozen and
 *     nomad_set_gemm_precision(ctx, 1) work.
 *   - Asynchronous; no allocation; the only host-to-device traffic is the metadata copy (a few ints per clip) queued on the
 *     stream ahead of the kernels.  Argument errors return their status before anything is queued.
 */
/* The per-clip metadata every ragged entry point derives from lengths_host and copies ahead of its kernels (pure host arithmetic, no
 * context): *count ints - [lengths (B) | then arrays of B + 1 prefix sums: frames per conv level 0..6 | padded pos-conv frames
 * (T_c + 128) | bf16x3 pos-conv blocks | output pairs of conv1..4 (ceil(L_i / 2)) | padded dU rows per level 0..6 (L_i + 2) |
 * even frames of levels 0..3 (ceil(L_i / 2)) | odd frames of levels 0..3 (floor(L_i / 2))].  out_host == NULL: the count only. */
int nomad_ragged_metadata(int B, const int* lengths_host, int* out_host, size_t capacity, size_t* count);
int nomad_saved_bytes_ragged(const nomad_ctx* ctx, int B, const int* lengths_host, size_t* bytes);
int nomad_backward_workspace_bytes_ragged(const nomad_ctx* ctx, int B, const int* lengths_host, size_t* bytes);
int nomad_train_workspace_bytes_ragged(const nomad_ctx* ctx, int B, const int* lengths_host, size_t* bytes);
int nomad_embed_train_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                             const float* head_w_dev, const float* head_b_dev, float* emb_dev, float* layers_dev,
                             void* saved_dev, size_t saved_bytes, void* workspace_dev, size_t workspace_bytes,
                             nomad_stream_t stream);
int nomad_embed_backward_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                                const float* head_w_dev, const float* head_b_dev, const float* layers_dev,
                                const void* saved_dev, size_t saved_bytes, const float* dlayers_dev, const float* demb_dev,
                                float* dwav_dev, void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
int nomad_train_backward_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                                const float* layers_dev, const void* saved_dev, size_t saved_bytes, const float* demb_dev,
                                void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
int nomad_l1_loss_ragged(nomad_ctx* ctx, const float* a_layers_dev, const float* b_layers_dev, const float* a_emb_dev,
                         const float* b_emb_dev, long long M, int B, float* loss_dev, void* scratch_dev,
                         nomad_stream_t stream);
int nomad_l1_loss_backward_ragged(nomad_ctx* ctx, const float* a_layers_dev, const float* b_layers_dev,
                                  const float* a_emb_dev, const float* b_emb_dev, long long M, int B,
                                  const float* upstream_dev, float* dlayers_dev, float* demb_dev, nomad_stream_t stream);

/* ---- the windowed head on the gradient path: differentiable scores over time ------------------------------------------------
 * nomad_embed_windows* gives one embedding per window of a clip from one forward; these calls make the windows differentiable
 * down to the waveform.  Window geometry (win, hop in frames), the order of the output rows and their number are those of
 * nomad_embed_windows* (nomad_num_windows); W_total = B W(T), or sum_c W(T_c) for a ragged batch.
 *
 *   nomad_embed_train_windows[_ragged]     = nomad_embed_train[_ragged] (saved_dev mandatory) with the windowed head as the last
 *                                            stage: emb_dev is [W_total][256], each row with the bits head_windows_kernel gives
 *                                            the window's frames (a window over a whole clip: the clip's nomad_embed_train*
 *                                            embedding).  layers_dev, saved_dev, the workspace and their sizes are those of
 *                                            nomad_embed_train[_ragged].
 *   nomad_windows_backward_scratch_bytes   the backward's scratch for n_windows = W_total windows: [n_windows][768] fp32, rounded
 *                                            up to 256 bytes.  NOMAD_ERR_INVALID for n_windows <= 0 or bytes == NULL.
 *   nomad_embed_windows_backward[_ragged]  = nomad_embed_backward[_ragged] with dlayers_dev = NULL and demb_dev [W_total][256], the
 *                                            gradient of the window embeddings, -> dwav_dev [B][n_samples] ([B][stride], zero
 *                                            behind every length).  The head stage is two launches without atomics: each window's
 *                                            gradient with respect to its time mean, spread over its n = min(win, T) frames
 *                                            (the time sum is recomputed in the forward's order, so the ReLU mask is the
 *                                            forward's), into scratch_dev; then frame t of a clip receives the sum of the rows of
 *                                            the windows that cover it, k ascending in one fp32 accumulator, and exact zeros when
 *                                            none does (a gap with hop > win, the tail behind the last full window).  Every row
 *                                            of the frame gradient and every row of scratch_dev in use is written before it is
 *                                            read: nothing needs clearing.  feature_grad_mult and the workspace size
 *                                            (nomad_backward_workspace_bytes[_ragged]) as in nomad_embed_backward[_ragged].
 *   nomad_window_cover                     the windows that cover frame t of a clip of T frames: *k_lo .. *k_hi with
 *                                            k_hi = min(W - 1, t / hop), k_lo = max(0, ceil((t - min(win, T) + 1) / hop));
 *                                            k_lo > k_hi for a frame no window covers (the return value is still 0).  Host
 *                                            arithmetic, no context - the helper the scatter kernel itself calls.
 *                                            NOMAD_ERR_INVALID for T, win or hop < 1, t outside [0, T) or a NULL output.
 *
 * Contract: asynchronous, no allocation; deterministic, the same bits run to run.  A clip's row of dwav_dev from the ragged call
 * does not depend on the batch it is in: it has the bits of the clip's own ragged call at B = 1 with that clip's rows of demb_dev
 * (the ragged calls never split K; the equal-length ones may, as nomad_embed_train / nomad_embed_backward do).
 * NOMAD_ERR_INVALID, before anything is queued: win or hop < 1; head_w_dev / head_b_dev not both set or both NULL; a NULL
 * mandatory pointer (everything but the head override); a cut encoder (nomad_set_encoder_depth); fine-tuning mode
 * (nomad_train_enable: its forward draws dropout and LayerDrop masks this backward does not replay); and whatever
 * nomad_embed_train* / nomad_embed_backward* refuse.  NOMAD_ERR_WORKSPACE: scratch, workspace or saved block too small.
 */
int nomad_window_cover(int T, int win, int hop, int t, int* k_lo, int* k_hi);
int nomad_windows_backward_scratch_bytes(long long n_windows, size_t* bytes);
int nomad_embed_train_windows(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, int win, int hop,
                              const float* head_w_dev, const float* head_b_dev, float* emb_dev, float* layers_dev,
                              void* saved_dev, size_t saved_bytes, void* workspace_dev, size_t workspace_bytes,
                              nomad_stream_t stream);
int nomad_embed_train_windows_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                                     int win, int hop, const float* head_w_dev, const float* head_b_dev, float* emb_dev,
                                     float* layers_dev, void* saved_dev, size_t saved_bytes, void* workspace_dev,
                                     size_t workspace_bytes, nomad_stream_t stream);
int nomad_embed_windows_backward(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, int win, int hop,
                                 const float* head_w_dev, const float* head_b_dev, const float* layers_dev,
                                 const void* saved_dev, size_t saved_bytes, const float* demb_dev, float* dwav_dev,
                                 void* scratch_dev, size_t scratch_bytes, void* workspace_dev, size_t workspace_bytes,
                                 nomad_stream_t stream);
int nomad_embed_windows_backward_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                                        int win, int hop, const float* head_w_dev, const float* head_b_dev,
                                        const float* layers_dev, const void* saved_dev, size_t saved_bytes,
                                        const float* demb_dev, float* dwav_dev, void* scratch_dev, size_t scratch_bytes,
                                        void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);

/* ---- the head over caller-given spans of frames: speech-only and per-turn embeddings, differentiable --------------------------
 * The windows calls pool the head over frames the library chooses (win frames every hop).  These pool it over frames the CALLER
 * names.  A span is frames [t0, t1) of one clip, 0 <= t0 < t1 <= T_c (one frame = 320 samples and sees 400).  A row is an ordered
 * list of one or more spans of the same clip, ascending and not overlapping (t1_i <= t0_{i+1}; touching is allowed); there is one
 * output embedding per row.  Different rows may overlap freely and a clip may have no row.  A row's embedding is the plain head
 * applied to the concatenation of its spans' frames as if they were a clip of their own: time mean over n = sum (t1 - t0) frames,
 * ReLU, Linear(768, 256), L2 normalisation.  The encoder saw the WHOLE clip, exactly as with windows: a row is not the embedding
 * of the excerpt alone.
 *
 * The table, all host memory that may be freed on return (its copy is staged like the ragged metadata):
 *   R                 rows, >= 1
 *   row_clip[R]       the clip of each row, in [0, B), not decreasing: the rows of a clip are contiguous
 *   row_ptr[R + 1]    row r pools spans row_ptr[r] .. row_ptr[r + 1] - 1; row_ptr[0] = 0, strictly increasing; S = row_ptr[R]
 *   spans[S][2]       (t0, t1) in frames of the row's clip
 *
 *   nomad_spans_scratch_bytes            the scratch of the three calls below for B clips, R rows and S spans: the table's device
 *                                        copy (with the per-clip row ranges), plus [R][768] fp32 when backward != 0.
 *                                        NOMAD_ERR_INVALID for B or R < 1, S < R or bytes == NULL.
 *   nomad_embed_spans_ragged             = nomad_embed_windows_ragged with the table in place of (win, hop): ONE forward of
 *                                        `precision`, emb_dev is [R][256] in table order.  Bit contracts: a row of one span
 *                                        [a, a + n) has the bits nomad_embed_windows* gives a window over those frames; a row
 *                                        whose spans concatenate to the whole clip ([0, T), or [0, 64), [64, T)) has the bits of
 *                                        the clip's plain embedding of that precision (chunks of 64 frames are counted from the
 *                                        row's first frame and run across span boundaries).
 *   nomad_embed_train_spans_ragged       = nomad_embed_train_windows_ragged with the table, plus the scratch (sized with
 *                                        backward = 0) for the table's device copy.
 *   nomad_embed_spans_backward_ragged    = nomad_embed_windows_backward_ragged with the table; demb_dev is [R][256]; scratch sized
 *                                        with backward = 1.  Two launches without atomics: each row's gradient with respect to
 *                                        its time mean, already divided by n (the time sum is recomputed in the forward's order,
 *                                        so the ReLU mask is the forward's), into the scratch; then frame t of clip b receives
 *                                        the sum of those of the rows of clip b that contain t, in ascending row order in one
 *                                        fp32 accumulator; a frame no row contains, and a clip without a row, gets exact zeros.
 *                                        Everything is written before it is read: nothing needs clearing.
 *   nomad_frame_energy                   energy_dev[frame t of clip c] = (sum_{i < 400} (double)x_c[320 t + i]^2) / 400, clips
 *                                        packed in order ([sum_c T_c] doubles): every product and sum in float64 in a fixed order,
 *                                        no atomics, a frame a function of its own 400 samples only.  No scratch.
 *                                        NOMAD_ERR_INVALID: a NULL pointer, B < 1, a clip longer than stride or shorter than a frame.
 *
 * Contract of the three nomad_embed_*spans* calls: as for the windows calls - precision preconditions (nomad_enable_bf16*,
 * nomad_enable_backward), workspace and saved sizes, statuses; the head override is fp32 only; asynchronous, no allocation (the
 * table's device copy lives in the caller's scratch); deterministic.  The ragged calls never split K, so a clip's rows and its
 * row of dwav_dev have the bits of its own B = 1 call.  NOMAD_ERR_INVALID before anything is queued, nomad_last_error naming the
 * entry point, the row and the span: R < 1; a NULL table pointer; row_clip decreasing or out of range; a row without a span;
 * t0 < 0, t1 > T_c or t0 >= t1; spans of a row overlapping or out of order; a cut encoder; fine-tuning mode (the two gradient
 * calls); and whatever the windows calls refuse.  NOMAD_ERR_WORKSPACE: scratch, workspace or saved block too small.
 */
int nomad_spans_scratch_bytes(int B, int R, int S, int backward, size_t* bytes);
int nomad_embed_spans_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host, int precision,
                             int R, const int* row_clip, const int* row_ptr, const int* spans, const float* head_w_dev,
                             const float* head_b_dev, float* emb_dev, void* scratch_dev, size_t scratch_bytes,
                             void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
int nomad_embed_train_spans_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host, int R,
                                   const int* row_clip, const int* row_ptr, const int* spans, const float* head_w_dev,
                                   const float* head_b_dev, float* emb_dev, float* layers_dev, void* saved_dev,
                                   size_t saved_bytes, void* scratch_dev, size_t scratch_bytes, void* workspace_dev,
                                   size_t workspace_bytes, nomad_stream_t stream);
int nomad_embed_spans_backward_ragged(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host, int R,
                                      const int* row_clip, const int* row_ptr, const int* spans, const float* head_w_dev,
                                      const float* head_b_dev, const float* layers_dev, const void* saved_dev,
                                      size_t saved_bytes, const float* demb_dev, float* dwav_dev, void* scratch_dev,
                                      size_t scratch_bytes, void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
int nomad_frame_energy(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host, double* energy_dev,
                       nomad_stream_t stream);

/* ---- NomadLoss with layer weights and per-utterance terms; the encoder cut at depth ------------------------
 * The reference's NomadLoss loops `for i in range(self.L)` (nomad.py:264, :276; L = 13): a caller who lowers L trains against the first
 * L terms only.  These entry points give that, a weight per term, and one loss per utterance - and let the encoder stop behind the
 * deepest layer the loss reads.  The 13-term mean of nomad_l1_loss[_ragged] and its kernels are untouched.
 *
 * nomad_l1_loss_weighted: both layouts of the layer tensors in one call - a_layers_dev / b_layers_dev are [12][M][768], M frames in
 * all, clip b's rows being frames_host[b] consecutive ones (HOST array of B counts, each >= 1, summing to M; NULL: M / B frames each,
 * i.e. [12][B][T][768]); a_emb_dev / b_emb_dev [B][256].
 *   S[i][b]       sum of fabsf(a - b) over clip b's rows of layer i (i = 12: its 256 embedding values): differences in fp32,
 *                 accumulated in fp64 over chunks of 16 frames counted from the clip's first frame, chunk sums folded in chunk order.
 *                 No atomics: identical run to run, and a function of the clip's own values only.
 *   weights_host  [13] fp32 on the HOST, finite, >= 0, not all 0 (term 12 is the embedding).  A weight of 0 means the term's tensors
 *                 are NOT READ (not multiplied by 0): behind a cut encoder they hold whatever the caller's buffer held, and the
 *                 pointers of tensors no term with a weight reads may be NULL.
 *   reduction     NOMAD_L1_PER_CLIP: loss_dev[b] = (float) sum_i w_i S[i][b] / n[i][b], n = T_b * 768 (256 for the embedding), [B];
 *                 NOMAD_L1_BATCH:    loss_dev[0] = (float) sum_i w_i (sum_b S[i][b]) / (sum_b n[i][b]) - the meaning of
 *                 nomad_l1_loss[_ragged], with weights.  i and b ascending, combined in fp64.
 *   terms_dev     optional [13][B] float64 (out): the per-clip means S / n; 0 where the weight is 0.  NULL: not wanted.
 *   scratch_dev   nomad_l1_weighted_scratch_bytes(M, B) bytes - a function of (M, B) only.
 * nomad_l1_loss_weighted_backward: dlayers_dev [12][M][768], rows of clip b in layer i = sign(a - b) * w_i / n * upstream (one
 * rounding) - per clip upstream_dev[b] ([B]) and n = n[i][b]; batch upstream_dev[0] and n = sum_b n[i][b]; demb_dev [B][256] by the
 * same rule.  `depth` (1 .. 12; below 12 every weight from `depth` on must be 0): layers below it with weight 0 are written as zeros,
 * layers at or above it are NOT WRITTEN; demb_dev is not written when w_12 = 0 and may then be NULL.
 * Contract: asynchronous, no allocation; the prefix sums of frames_host are copied into the scratch ahead of the kernels, as the
 * ragged entry points queue their metadata; argument errors return their status before anything is queued.  Per clip, loss[b] and the
 * clip's rows of dlayers depend on that clip's values only: on the outputs of the ragged forward (which never splits K) loss[b] is
 * the bits of the clip's own B = 1 call.
 */
enum { NOMAD_L1_BATCH = 0, NOMAD_L1_PER_CLIP = 1 };
int nomad_l1_weighted_scratch_bytes(long long M, int B, size_t* bytes);
int nomad_l1_loss_weighted(nomad_ctx* ctx, const float* a_layers_dev, const float* b_layers_dev, const float* a_emb_dev,
                           const float* b_emb_dev, long long M, int B, const int* frames_host, const float* weights_host,
                           int reduction, float* loss_dev, double* terms_dev, void* scratch_dev, size_t scratch_bytes,
                           nomad_stream_t stream);
int nomad_l1_loss_weighted_backward(nomad_ctx* ctx, const float* a_layers_dev, const float* b_layers_dev, const float* a_emb_dev,
                                    const float* b_emb_dev, long long M, int B, const int* frames_host, const float* weights_host,
                                    int reduction, int depth, const float* upstream_dev, float* dlayers_dev, float* demb_dev,
                                    void* scratch_dev, size_t scratch_bytes, nomad_stream_t stream);
/*
 * Encoder depth, per context like nomad_set_feature_grad_mult: 1 .. 12, default 12.  While it is k < 12
 *   - nomad_embed WITH layers_dev, nomad_embed_train and nomad_embed_train_ragged run the conv stack, the projection, the pos-conv and
 *     encoder layers 0 .. k - 1, then stop: rows [k, 12) of layers_dev and emb_dev are not written, the head is not launched.
 *     Workspace and saved-block sizes stay functions of the geometry (their tail is unused);
 *   - nomad_embed_backward[_ragged] start at layer k - 1 with dlayers_dev[k - 1] as the only incoming gradient: no head backward,
 *     demb_dev is ignored and may be NULL, rows >= k of dlayers_dev are not read, dlayers_dev itself is required;
 *   - every other forward and the fine-tuning backward return NOMAD_ERR_INVALID with a message that names the depth (nomad_embed without
 *     layers_dev, nomad_embed_ragged, nomad_embed_features*, every bf16 / bf16x3 entry point, nomad_train_backward*): a truncated
 *     encoder behind a score or a fine-tuning step is never a silent result.
 * Bits: with loss weights that are 0 from layer k on (w_12 = 0 too) layer outputs 0 .. k - 1, the loss and dwav of the run at depth k
 * are those of the run at depth 12 - there the upper layers only propagate exact zeros - and the equal-length path's split-K choice
 * depends on the batch's frames, not on the depth.
 */
int nomad_set_encoder_depth(nomad_ctx* ctx, int depth);
int nomad_get_encoder_depth(const nomad_ctx* ctx, int* depth);

/* ---- triplet fine-tuning step (src/training/train_triplet.py:112-133, src/config/train_triplet.yaml) ---- */
/*
 * The reference fine-tunes wav2vec 2.0 + head with A/P/N forwards, nn.TripletMarginLoss(margin),
 * loss.backward() and Adam (1e-5 on the backbone, `lr` on embedding_layer), conv feature extractor frozen
 * (freeze_convnet: True, the shipped config; False is supported too).  Here the trainable parameters live in ONE flat fp32 device vector (master copy in
 * checkpoint layout), with gradients and the two Adam moments in vectors of the same layout:
 *
 *   nomad_train_param_count   floats in the vector; head_begin = first float of embedding_layer (own lr)
 *   nomad_train_num_segments / nomad_train_segment   checkpoint key -> (offset, count) of the vector
 *   nomad_train_enable        allocates the vectors, fills the parameters from `host_weights` (the same struct
 *                             nomad_create took), re-points the engine at them (also calls nomad_enable_backward)
 *   nomad_train_zero_grad     gradients = 0
 *   nomad_embed_train         (above) forward that saves activations
 *   nomad_train_backward      given d loss / d emb [B][256]: ACCUMULATES d loss / d parameters into the gradient
 *                             vector (dW as MFMA GEMMs, split over the B*T contraction, fixed-order reduction);
 *                             scratch: nomad_train_workspace_bytes.  Stops at the feature extractor unless
 *                             nomad_train_set_convnet made it trainable.
 *   nomad_triplet_loss        loss [1] = mean_i max(||a-p+eps|| - ||a-n+eps|| + margin, 0), eps = 1e-6
 *                             (torch.pairwise_distance); da/dp/dn [B][256] nullable together (validation pass)
 *   nomad_train_adam_step     torch.optim.Adam update (amsgrad off, no weight decay) with the step count kept in
 *                             the context, then rebuilds the derived kernel-layout weights.  beta1 / beta2 are doubles:
 *                             1 - beta and 1 - beta^t are formed in double (1.0f - 0.999f is off by 1.3e-5 relative)
 *   nomad_train_read / write  copy a whole vector out of / into the context (device pointers, async on stream);
 *                             what: 0 parameters, 1 gradients, 2 exp_avg, 3 exp_avg_sq
 *   nomad_train_set_step      set Adam's step counter (resume)
 *   nomad_train_set_stochastic   model.train() regularisation for the following nomad_embed_train /
 *                             nomad_train_backward calls: fairseq's dropout (after the encoder LayerNorm, out_proj
 *                             and fc2), attention_dropout (softmax probabilities), dropout_input (after
 *                             post_extract_proj) and LayerDrop (layer_mask bit l clear = layer l skipped).  Masks are a
 *                             counter-based hash of (seed, site, element): set the SAME values before a forward
 *                             and before its backward.  All zero + mask 0xFFF (the default) = eval-mode arithmetic.
 *   nomad_train_set_frozen    freeze_encoder != 0: the reference's `freeze_all: True` (train_triplet.py:76-79) - the conv feature
 *                             extractor AND the encoder (pos-conv, encoder LayerNorm, 12 layers) are frozen; gradients still
 *                             flow through them to post_extract_proj and the feature LayerNorm, which stay trainable with
 *                             the head.  Frozen parameters keep a zero gradient, so the Adam step leaves them untouched.
 *   nomad_train_set_convnet   trainable != 0: the reference's `freeze_convnet: False` (train_triplet.py:71-73) - the conv
 *                             feature extractor's weights and its GroupNorm get gradients too (conv dW as split-K MFMA GEMMs
 *                             over transposed im2col operands; scaled by feature_grad_mult like every gradient that
 *                             enters the extractor); changes nomad_train_workspace_bytes.  Default 0: their slices of the
 *                             gradient vector stay zero.
 *   nomad_train_set_branches  the batch of the following nomad_embed_train / nomad_train_backward calls is `branches`
 *                             equal groups of clips (anchor | positive | negative), each with its own LayerDrop mask -
 *                             as if each group had been its own forward call, but one launch sequence over all of
 *                             them wherever the masks agree.  branches = 1 (default): layer_mask of set_stochastic.
 */
int nomad_train_param_count(size_t* total, size_t* head_begin);
int nomad_train_num_segments(void);
int nomad_train_segment(int i, char* name, size_t name_cap, size_t* offset, size_t* count);
int nomad_train_enable(nomad_ctx* ctx, const nomad_weights* host_weights);
int nomad_train_workspace_bytes(const nomad_ctx* ctx, int B, int n_samples, size_t* bytes);
int nomad_train_zero_grad(nomad_ctx* ctx, nomad_stream_t stream);
int nomad_train_backward(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, const float* layers_dev,
                         const void* saved_dev, size_t saved_bytes, const float* demb_dev,
                         void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
int nomad_triplet_loss(nomad_ctx* ctx, const float* a_dev, const float* p_dev, const float* n_dev, int B,
                       float margin, float* loss_dev, float* da_dev, float* dp_dev, float* dn_dev,
                       nomad_stream_t stream);
int nomad_train_adam_step(nomad_ctx* ctx, float lr_body, float lr_head, double beta1, double beta2, float eps,
                          nomad_stream_t stream);
int nomad_train_read(nomad_ctx* ctx, int what, float* dst_dev, nomad_stream_t stream);
int nomad_train_write(nomad_ctx* ctx, int what, const float* src_dev, nomad_stream_t stream);
int nomad_train_set_step(nomad_ctx* ctx, long long step);
int nomad_train_set_stochastic(nomad_ctx* ctx, float dropout, float attention_dropout, float dropout_input,
                               unsigned long long seed, unsigned layer_mask);
int nomad_train_set_branches(nomad_ctx* ctx, int branches, const unsigned* layer_masks);
int nomad_train_set_frozen(nomad_ctx* ctx, int freeze_encoder);
int nomad_train_set_convnet(nomad_ctx* ctx, int trainable);

/* ---- degradations on packed clips: noise at an SNR, percentile clipping ----------------------------------------------
 * The two degradations of the reference's src/utils/degradations.py that are arithmetic on samples, G levels of each per clip in one
 * call, written straight into the layout nomad_embed_ragged reads.  x_dev is [B][stride] fp32, clip b in the first lens_host[b]
 * samples of its row (the rest of the row is never read); lens_host and the levels are HOST arrays; out_dev is [B G][stride] fp32:
 * row b G + g is clip b at level g, with length lens_host[b]; every row is zero behind its length.
 *
 * nomad_degrade_noise (degradations.py:30-68), per clip of n samples, noise s of noise_len samples on the device, all in float64:
 *   xp = sqrt(mean_i x[i]^2),  sp = sqrt(mean_i s[i mod noise_len]^2), both over i < n (the noise tiled or cut to the clip),
 *   alpha = (xp / 10^(snr_db[g] / 10)) / sp,   out[i] = (float)((double)x[i] + alpha * (double)s[i mod noise_len])
 * - the reference's formula as it stands: an amplitude divided by a power ratio.  10^(snr_db / 10) is formed on the host (pow).  The
 * sums of squares are float64, one workgroup per clip: thread t of 1024 adds samples t, t + 1024, ... in order, the 1024 partial sums
 * fold by halves; product and sum of the output are rounded separately.  No special cases: a silent clip or silent noise gives what
 * IEEE arithmetic gives (0, inf or NaN).  alpha_out_dev: optional [B][G] float64 (out), or NULL.
 *
 * nomad_degrade_clip (degradations.py:70-83): per level p_lo = clip_factor[g] / 2 and p_hi = 100 - clip_factor[g] / 2, a percentile p
 * being numpy's default linear rule on the clip's own samples, in float64:
 *   h = (n - 1) (p / 100.0), lo = floor(h), hi = min(lo + 1, n - 1), t = h - lo, v = a + (b - a) t  (two roundings, no fused
 *   multiply-add), a and b the lo-th and hi-th order statistics of the clip in numpy's sort order (NaN last);
 *   out[i] = x > v_hi ? (float)v_hi : x < v_lo ? (float)v_lo : x, compared in float64 (a NaN threshold leaves the samples as they are).
 * The order statistics are exact: each clip is radix-sorted (4 passes of 8 bits, stable) into the workspace.
 * thresholds_out_dev: optional [B][G][2] float64 (out): (v_lo, v_hi), or NULL.
 *
 * Contract: asynchronous, no allocation; the levels and lengths are copied into the workspace ahead of the kernels, as the ragged
 * entry points queue their metadata.  Deterministic, no floating-point atomics; a clip's rows, alpha and thresholds do not depend on
 * the batch: they have the bits of the clip's own B = 1 call.  Workspace: nomad_degrade_scratch_bytes(B, stride, G) bytes (0 for
 * arguments the calls would refuse), written before it is read.  Argument errors return before anything is queued.
 * NOMAD_ERR_INVALID: a NULL pointer other than the optional output, G outside 1 .. 64, B < 1 (or above 65535), stride not a positive
 * multiple of 4 or shorter than a length, a length < 1, noise_len < 1, a clip_factor outside [0, 100], a level that is not finite.
 * NOMAD_ERR_WORKSPACE: ws_bytes too small.
 */
size_t nomad_degrade_scratch_bytes(int B, int stride, int G);
int nomad_degrade_noise(nomad_ctx* ctx, const float* x_dev, int B, int stride, const int* lens_host, const float* noise_dev,
                        int noise_len, const double* snr_db_host, int G, float* out_dev, double* alpha_out_dev,
                        void* ws_dev, size_t ws_bytes, nomad_stream_t stream);
int nomad_degrade_clip(nomad_ctx* ctx, const float* x_dev, int B, int stride, const int* lens_host, const double* clip_factor_host,
                       int G, float* out_dev, double* thresholds_out_dev, void* ws_dev, size_t ws_bytes, nomad_stream_t stream);

/* ---- reverberation on packed clips: every clip convolved with G impulse responses --------------------------------------
 * For any fixed setting a reverberator is a linear, time-invariant filter.  x_dev is [B][stride] fp32 with lens_host as above; ir_dev
 * is [G][ir_stride] fp32, response g in the first ir_lens_host[g] taps of its row (the rest of either row is never read: anything,
 * NaN included, may stand there); the G responses are applied to EVERY clip.  out_dev is [B G][stride] fp32, row b G + g being clip b
 * through response g, causal and cut to the clip's length n_b (sox's effect chain leaves the same):
 *   out[b G + g][i] = sum_{k = 0}^{min(L_g - 1, i)} h_g[k] x_b[i - k]   for i < n_b,      0 for n_b <= i < stride.
 * Arithmetic: fp32 products, fp32 accumulation, no fp32 rounding skipped or added (v_mfma_f32_16x16x4_f32, an fmaf chain).  Order as
 * built: the taps in chunks of 241 (k = 0 .. 240, 241 .. 481, ...) in ascending order, inside a chunk from its LAST tap down to its
 * first, one chain per output; samples before the clip's start and the taps a chunk lacks enter as zeros (products with them are
 * formed and add +-0).  The order depends on (n_b, L_g) and the output's index only: row b G + g of any batch has the bits of the
 * clip's own B = 1, G = 1 call.  Integer-valued inputs whose partial sums stay below 2^24 give the exact sums.
 * Non-finite values: a non-finite sample at position p of clip b makes out[b G + g][p .. min(p + L_g, n_b) - 1] non-finite for every
 * g, a non-finite tap k makes out[b G + g][k .. n_b - 1] non-finite for every b; no row of another clip and, for a tap, no row of
 * another response changes.  Within the affected row FURTHER samples may turn non-finite (0 x NaN against a padding zero of a
 * 16 x 256 Toeplitz tile: up to 255 outputs around the formula's range, and outputs ahead of a bad tap).
 * Contract as the degradations above: asynchronous, no allocation, deterministic; the two length tables are copied into the
 * workspace ahead of the kernel; workspace nomad_degrade_convolve_scratch_bytes(B, G) bytes (0 for arguments the call would refuse),
 * written before it is read.  Argument errors return before anything is queued.
 * NOMAD_ERR_INVALID: a NULL pointer, G outside 1 .. 64, B < 1 (or above 65535), stride or ir_stride not a positive multiple of 4 or
 * shorter than a length, a clip length < 1, a response length outside 1 .. 65536 (4.096 s at 16 kHz).
 * NOMAD_ERR_WORKSPACE: ws_bytes too small.
 */
size_t nomad_degrade_convolve_scratch_bytes(int B, int G);
int nomad_degrade_convolve(nomad_ctx* ctx, const float* x_dev, int B, int stride, const int* lens_host, const float* ir_dev, int G,
                           int ir_stride, const int* ir_lens_host, float* out_dev, void* ws_dev, size_t ws_bytes,
                           nomad_stream_t stream);

/* ---- loudness normalisation of packed rows: ITU-R BS.1770-4 (mono), linear gain to a target ------------------------------
 * The reference's rendering scripts follow every degraded file with `ffmpeg-normalize FILE -o FILE -f -ar 16000`: EBU R128, integrated
 * loudness brought to -23 LUFS, so that its intensity experiment ranks degradations at equal loudness.  This call measures R packed
 * rows and scales each by ONE gain, in place if wanted.  x_dev is [R][stride] fp32, row r in its first lens_host[r] samples (the rest
 * is never read); lens_host is a HOST array.
 *
 * K-weighting: two cascaded biquads in transposed direct form II, state and output float64, coefficients formed on the host in
 * float64 from sample_rate = fs:
 *   shelf:     f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *              Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *              b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *   high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, same K and a0 forms, b = [1, -2, 1], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 * (at 48 kHz the standard's table).  Blocks: hop = fs / 10 samples, block j covers filtered samples [j hop, j hop + 4 hop) (400 ms,
 * 75 % overlap); only whole blocks count: nb = (n - 4 hop) / hop + 1 for n >= 4 hop, else 0; z_j = mean square of block j,
 * l_j = -0.691 + 10 log10 z_j.  Gating: absolute l_j > -70; relative Gamma = -0.691 + 10 log10(mean z_j over the absolute-gated
 * blocks) - 10; L = -0.691 + 10 log10(mean z_j over the blocks with l_j > -70 and l_j > Gamma); L = -inf if no block passes the
 * absolute gate (digital silence, any row shorter than 400 ms).
 * mode 0 (ebu): the level is L, in LUFS; 1 (rms): 20 log10 sqrt(mean x^2) over the row, dBFS; 2 (peak): 20 log10 max|x|, dBFS -
 * ffmpeg-normalize -nt's three.  The peak, measured in every mode, is the SAMPLE peak max|x|, not the 4x oversampled true peak.
 * Gain: g = 10^((target - level) / 20) in float64; with a ceiling peak_db (NaN: none) g = min(g, 10^(peak_db / 20) / peak);
 * out[i] = (float)((double)x[i] g) for i < n, zero behind the length.  A row whose level is -inf is copied unchanged (g = 1, no
 * ceiling).  This is the LINEAR gain of ffmpeg's loudnorm; its dynamic mode, loudness-range target and true-peak limiter are not offered.
 *
 * How the recurrence runs in parallel (csrc/loudness.hip.h): the row is cut into chunks of hop samples, each walked from a zero
 * state, the true entry states follow from s_{j+1} = M s_j + e_j (M: the cascade's 4 x 4 transition over hop samples, from the host),
 * each whole chunk is walked again from its true state for its sum of y^2, and block j is chunks j .. j + 3 added in that order.
 * Every sum is float64 in an order fixed by (n, fs): a row's statistics and output have the bits of its own R = 1 call.
 * out_dev: [R][stride] fp32; may be x_dev exactly (in place), or NULL (measure only).  stats_out_dev: optional [R][4] float64 =
 * (level, sample peak, applied gain, blocks that passed both gates - 0 in the rms and peak modes), or NULL.
 * Non-finite input: a NaN or infinite sample makes its row's level, gain and block count NaN, its peak NaN or inf and its output
 * samples [0, n) NaN; no other row changes, and zeros stay behind the length.
 * Contract as the degradations above: asynchronous, no allocation, deterministic, no floating-point atomics; the lengths are copied
 * into the workspace ahead of the kernels; workspace nomad_degrade_normalize_scratch_bytes(R, stride, sample_rate) bytes (0 for
 * arguments the call would refuse), written before it is read.  Argument errors return before anything is queued.
 * NOMAD_ERR_INVALID: a NULL x_dev (context, lengths, workspace), both outputs NULL, R outside 1 .. 65535, stride not a positive
 * multiple of 4 or shorter than a length, a length < 1, sample_rate outside 8000 .. 192000 or no multiple of 10, mode outside 0 .. 2,
 * a target that is not finite, out_dev overlapping x_dev other than exactly.  NOMAD_ERR_WORKSPACE: ws_bytes too small.
 */
size_t nomad_degrade_normalize_scratch_bytes(int R, int stride, int sample_rate);
int nomad_degrade_normalize(nomad_ctx* ctx, const float* x_dev, int R, int stride, const int* lens_host, int sample_rate, int mode,
                            double target, double peak_db, float* out_dev, double* stats_out_dev, void* ws_dev, size_t ws_bytes,
                            nomad_stream_t stream);

/* ---- sox-style reverb on packed clips: the Freeverb comb and all-pass recurrences, G reverberance levels per clip --------
 * The reference renders its REVERB conditions with sox's `reverb P` (src/utils/degradations.py), P = reverberance in 0 .. 100.
 * nomad_degrade_convolve above cannot stand in for it: at P = 100 the comb feedback is 0.98 on loops of about 500 samples, and
 * after 65536 taps the response has fallen by only about 25 dB.  This call runs the reverberator itself.
 *
 * WHAT THIS IS NOT: a port checked against sox.  The algorithm below is restated from memory of sox 14.4 reverb.c; neither sox
 * nor torchaudio was available where it was written, so its agreement with the sox binary has never been measured.  The text
 * below is the definition, and tests/freeverb_ref.py restates it sample by sample.
 *
 * Parameters (sox's names; range; sox's default): reverberance[g] 0 .. 100 (50), hf_damping 0 .. 100 (50), room_scale 0 .. 100 (100),
 * stereo_depth 0 .. 100 (100), pre_delay_ms 0 .. 500 (0), wet_gain_db -10 .. 10 (0), wet_only 0 / 1 (0).  fs = sample_rate.
 * All of the following is float64:
 *   a = -1 / ln(1 - 0.3);  b = 100 / (ln(1 - 0.98) a + 1);  feedback = 1 - exp((reverberance - b) / (a b))
 *   damp = hf_damping / 100 * 0.3 + 0.2;  gain = 10^(wet_gain_db / 20) * 0.015
 *   scale = room_scale / 100 * 0.9 + 0.1;  depth = stereo_depth / 100;  r = fs * (1 / 44100.)
 *   pre = (int)(pre_delay_ms / 1000 * fs + 0.5)
 *   comb lengths {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617};  all-pass {225, 341, 441, 556};  stereo adjust 12
 *   channels c = 0 .. ceil(depth):  off = c * depth, its sign flipping after EVERY filter, combs first, then the all-passes:
 *       comb i:      D = (int)(scale * r * (len_i + 12 * off) + 0.5);  off = -off
 *       all-pass j:  D = (int)(        r * (len_j + 12 * off) + 0.5);  off = -off      (not scaled by the room)
 * (16 kHz, defaults: channel 0 combs 405 431 463 492 516 541 565 587, all-passes 82 124 160 202; channel 1 combs 409 427 468 488 520
 * 537 569 582, all-passes 86 119 164 197; feedback 0.3 at reverberance 0, 0.8816784043380077 at 50, 0.98 at 100.)
 * Per channel and sample t, in = x[t - pre] (0 before the start), every delay line and store starting at zero:
 *   acc = 0;  for i = 7 down to 0:  o = line_i[t - D_i];  store_i = o + (store_i - o) * damp;
 *                                    line_i[t] = in + store_i * feedback;  acc += o
 *   for j = 3 down to 0:  o = ap_j[t - D_j];  ap_j[t] = acc + o * 0.5;  acc = o - acc
 *   wet_c[t] = acc * gain
 * The clip is mono and so is the row: y[t] = (1 - wet_only) x[t] + mean_c wet_c[t] (two channels: 0.5 (wet_0 + wet_1); stereo_depth = 0:
 * one channel), cut to the clip's length - no tail, as nomad_degrade_convolve.  With clamp != 0 the result is limited as sox's sample
 * conversion does, v > 1 ? 1 : v < -1 ? -1 : v (a NaN stays a NaN); then ONE rounding to fp32.
 *
 * x_dev is [B][stride] fp32 with lens_host as above (nothing behind a length is read); out_dev is [B G][stride] fp32, row b G + g
 * being clip b at params->reverberance[g], zeros from its length to the stride; the other parameters are shared by the call.
 * How it runs (csrc/reverb.hip.h): a workgroup per (row, channel), a wave per comb with its delay line as a ring in LDS, time in
 * tiles of T = min(64, the call's shortest delay) samples - one per lane - inside which only the one-pole `store` is a chain: a
 * fixed-order scan across the lanes; a ninth wave adds the combs' outputs in the order 7 .. 0 and runs the all-passes; the wet
 * signal of each channel goes to the workspace as float64 and a second kernel mixes, limits and rounds.  State and arithmetic are
 * float64, there are no atomics, and every order is fixed by the clip's length and the shared parameters: row b G + g has the bits of
 * the clip's own B = 1, G = 1 call.  Against the sample-by-sample recurrence the scan reassociates (a few units of 2^-53 per
 * sample, amplified by at most 1 / (1 - feedback) <= 50).
 * Non-finite input: a non-finite sample at position p of clip b makes every row of b non-finite at p (and, through the loops,
 * possibly anywhere from there on); outputs at indices below p - p % 64 keep the bits of the clean run; no row of another clip
 * changes; zeros stay behind every length.  (With clamp != 0 it is a NaN that stays: an infinite value is limited to +-1 like any
 * other value beyond the range, as the formula above says.)
 * Contract as the degradations above: asynchronous, no allocation, deterministic, the caller's stream; the lengths and the
 * parameters are copied (the struct is read during the call, the tables go into the workspace ahead of the kernels), so both host
 * objects may die on return.  Workspace: nomad_degrade_reverb_scratch_bytes(B, stride, G, sample_rate) bytes (0 for arguments the
 * call would refuse) = two small tables + 16 bytes per output sample, written before it is read.  Argument errors return before
 * anything is queued.
 * NOMAD_ERR_INVALID: a NULL pointer, G outside 1 .. 64, B outside 1 .. 65535, stride not a positive multiple of 4 or shorter than a
 * length, a length < 1, a parameter outside its range above or not finite, sample_rate outside 8000 .. 48000, out_dev overlapping
 * x_dev.  NOMAD_ERR_WORKSPACE: ws_bytes too small.
 */
typedef struct {
    int G;
    double reverberance[64];
    double hf_damping, room_scale, stereo_depth, pre_delay_ms, wet_gain_db;
    int wet_only, clamp, sample_rate;
} nomad_reverb_params;
size_t nomad_degrade_reverb_scratch_bytes(int B, int stride, int G, int sample_rate);
int nomad_degrade_reverb(nomad_ctx* ctx, const float* x_dev, int B, int stride, const int* lens_host, const nomad_reverb_params* params_host,
                         float* out_dev, void* ws_dev, size_t ws_bytes, nomad_stream_t stream);

/* ---- gammatone spectrograms of packed rows and their NSIM: the similarity the reference's triplets are sampled from ----------
 * The reference runs ViSQOL over every (clean, degraded) pair and builds its (Anchor, Positive, Negative) rows from the pairs' NSIM
 * (src/utils/nsim_triplet_sampling.py).  These calls compute a gammatone-spectrogram NSIM over the packed rows the nomad_degrade_*
 * calls write, so that triplets can be mined with nothing rendered to disk.
 *
 * WHAT THIS IS NOT: a port checked against ViSQOL.  The measure below is modelled on what ViSQOL's speech mode is remembered to do
 * (Slaney's ERB gammatone bank, 80 ms frames every 20 ms with the filter state reset per frame, dB floors, a 3 x 3 NSIM window);
 * ViSQOL was not available where it was written, so its agreement with the ViSQOL binary has never been measured.  The text
 * below is the definition, and tests/nsim_ref.py restates it.  These two calls have no patch search and no voice-activity gate
 * (nomad_nsim_patches below adds both, over whole frames), and
 * they align nothing: one similarity map covers the whole clip, so the rows must be sample-aligned with their clean clip.
 * The rows the degradations make are, by construction; rows with ONE constant delay of whole samples (a codec round trip, a model
 * with latency) are brought there by nomad_align_delay / nomad_align_shift below.  Delays that change inside a file (clock drift, dropped
 * packets) are followed in steps of whole frames by nomad_nsim_patches.  Still outside what is claimed: sub-sample delays, and
 * agreement with ViSQOL's own aligner, which has not been measured.  No MOS mapping.  The gradient of these two calls with respect
 * to the degraded rows is nomad_nsim_backward / nomad_gammatone_backward ("NSIM as a loss" below).
 *
 * Rows are fp32, mono, at fs = sample_rate samples per second, fs in 16000 .. 48000 and a multiple of 50.  Everything below is float64.
 * Bank: N = 21 bands.  With EarQ = 9.26449, minBW = 24.7, lo = 50, hi = 8000:
 *   cf_i = -EarQ minBW + exp(i (log(lo + EarQ minBW) - log(hi + EarQ minBW)) / N) (hi + EarQ minBW) for i = 1 .. N; band 0 is the
 *   lowest (i = N, 50 Hz), band 20 the highest (i = 1).
 *   T = 1 / fs, ERB = cf / EarQ + minBW, B = 1.019 2 pi ERB, c = cos(2 pi cf T), s = sin(2 pi cf T), e = exp(B T).
 *   Four second-order sections with the common denominator [1, -2 c / e, exp(-2 B T)] and the numerators [T, A1k, 0],
 *   A1k = -(2 T c / e +- 2 sqrt(3 +- 2^1.5) T s / e) / 2 in the order (+,+), (-,+), (+,-), (-,-): the first sign is the one in front
 *   of the square root, the second the one inside it.  The gain g is the magnitude of the product of the four sections' responses at
 *   z = exp(j 2 pi cf T), formed on the host in complex float64; it is divided into the first section's two numerator coefficients
 *   on the host.  Each section runs as transposed direct form II: y = b0 x + z1; z1 = b1 x - a1 y + z2; z2 = -a2 y.  All
 *   coefficients are formed on the host, once per call.
 * Spectrogram: W = 0.08 fs = 4 H, H = 0.02 fs.  A row of n >= W samples has F = (n - W) / H + 1 whole frames (integer division;
 *   nomad_gammatone_frames(n, fs), <= 0 for a shorter row or a rate outside the range); a trailing partial frame is in none.  For
 *   frame t and band b the four sections run over samples [t H, t H + W) from the zero state, section k fed by section k - 1, and
 *   S[t][b] = sqrt((sum_i y_i^2) / W), the sum taken in time order.  Frames are packed clip after clip as [sum F_r][21] doubles,
 *   as nomad_frame_energy packs its frames.
 * NSIM of a clean spectrogram R and a degraded one D with the same F: eps = 2^-52; X = 10 log10(max(S, eps)); the absolute floor
 *   X = max(X, -45); for each frame X_t = max(X_t, p_t - 45), p_t the largest value of frame t in either spectrogram; then the
 *   smallest value left in either is subtracted from both.  The window is w = [[0.0113, 0.0838, 0.0113], [0.0838, 0.6193, 0.0838],
 *   [0.0113, 0.0838, 0.0113]], applied with the edges replicated so that the map stays F x 21, its nine terms added row by row:
 *   frames t - 1, t, t + 1 outside, bands b - 1, b, b + 1 inside.  mu = w * X; variance = w * X^2 - mu^2 clamped at 0, sigma its
 *   square root; covariance = w * (R D) - mu_R mu_D.  C1 = (0.01 L)^2 and C3 = (0.03 L)^2 / 2 with the intensity range L a call
 *   parameter (1.0 where a caller has no reason for another).  The map is
 *   (2 mu_R mu_D + C1) / (mu_R^2 + mu_D^2 + C1) * ((cov + C3) / (sigma_R sigma_D + C3)).
 *   A band's value is the mean of its column over the F frames, added in ascending order (a sequential walk); the row's NSIM is the
 *   mean of the 21 band values, added in ascending order.
 * Non-finite samples: a non-finite sample makes every frame that holds it NaN; every max and min above is formed so that a NaN
 *   sticks, so that row's NSIM and band values are NaN, and no other row changes a bit.  A silent pair gives exactly 1.
 *
 *   nomad_gammatone   x_dev [R][stride] fp32, row r in its first lens_host[r] samples (HOST array; nothing behind a length is read,
 *                     rows need 4-byte alignment only) -> spec_out_dev [sum F_r][21] float64.  A (frame, band) value depends on its
 *                     own W samples and the rate alone: a row has the bits of its own R = 1 call whatever the batch, the stride
 *                     and the base alignment.  csrc/nsim.hip.h states how the work is laid out (a lane per (frame, band), a
 *                     workgroup's span of samples staged in LDS once, the cascade skewed by one sample per section).
 *   nomad_nsim        spec_ref_dev [sum F_b][21] (B clean clips), spec_deg_dev [G sum F_b][21]: degraded row b G + g belongs to clean
 *                     clip b and has its F_b = frames_host[b] frames, rows packed in that order -> nsim_out_dev [B G], bands_out_dev
 *                     [B G][21] or NULL (the scores keep their bits).  One workgroup per degraded row; a row has the bits of its
 *                     own B = 1, G = 1 call.
 * Contract as the degradations above: asynchronous on the caller's stream, no allocation, deterministic, no atomics; the host
 * tables (lengths or frame counts, their prefix sums, the bank) are copied into the workspace ahead of the kernels, so the host
 * arrays may die on return; workspace nomad_gammatone_scratch_bytes(R, stride, sample_rate) / nomad_nsim_scratch_bytes(B, G,
 * total_frames = sum F_b) bytes (0 for arguments the call would refuse), written before it is read.  Argument errors return before
 * anything is queued.
 * NOMAD_ERR_INVALID: a NULL pointer other than bands_out_dev, R or B outside 1 .. 65535, G outside 1 .. 64, a stride that is not a
 * positive multiple of 4 or is shorter than a length, a length below one frame, a rate outside the range above, a frame count
 * below 1, an intensity range that is not finite and positive.  NOMAD_ERR_WORKSPACE: ws_bytes too small.
 */
int nomad_gammatone_frames(int n_samples, int sample_rate);
size_t nomad_gammatone_scratch_bytes(int R, int stride, int sample_rate);
int nomad_gammatone(nomad_ctx* ctx, const float* x_dev, int R, int stride, const int* lens_host, int sample_rate, double* spec_out_dev,
                    void* ws_dev, size_t ws_bytes, nomad_stream_t stream);
size_t nomad_nsim_scratch_bytes(int B, int G, long long total_frames);
int nomad_nsim(nomad_ctx* ctx, const double* spec_ref_dev, const double* spec_deg_dev, int B, int G, const int* frames_host /* [B] */,
               double intensity_range, double* nsim_out_dev /* [B G] */, double* bands_out_dev /* [B G][21] or NULL */, void* ws_dev,
               size_t ws_bytes, nomad_stream_t stream);

/* ---- NSIM as a loss: the gradient of nomad_nsim and nomad_gammatone with respect to the degraded (estimated) rows --------------
 * The whole-clip measure above, differentiated: d nsim[j] / d spec_deg (nomad_nsim_backward) and from there down to the samples of
 * the degraded rows (nomad_gammatone_backward).  The clean rows get no gradient.  The patch search, the alignment and everything
 * else in this header that says so stay without one.  The measure is this project's: its agreement with ViSQOL is not measured,
 * and neither is that of its gradient with any differentiable ViSQOL.  All quantities are float64; the samples' gradient is rounded
 * to fp32 once.
 *
 * The measure has maxima, a minimum, a clamp and square roots; these conventions make its gradient finite (digital silence
 * included) and are the definition.  tests/nsim_grad_ref.py restates them.
 *   Square roots: S = sqrt(acc / W) has gradient 0 where acc == 0; sigma = sqrt(var) has gradient 0 where var <= 0 (clamped or
 *     exactly zero).
 *   Floors: every max(value, floor) passes its gradient to value only where value > floor strictly; otherwise it goes to the
 *     floor.  The constants eps and -45 take nothing; the per-frame floor p_t - 45 hands it to p_t.
 *   Peak: p_t passes its gradient to the FIRST cell that attains it in the forward's own order: clean bands ascending, then
 *     degraded bands ascending (a later cell replaces an earlier one only where it is strictly greater).  If that cell is a clean
 *     one the gradient ends there.  Clean cells on p_t - 45 do hand their gradient to a degraded peak: the clean plane's
 *     derivative is carried up to this step.  p_t's gradient is the sum over the clean cells on the frame's floor in ascending
 *     bands, then the degraded ones in ascending bands.
 *   Least: the smallest value left in either plane receives -sum(dR + dD) over all cells of both planes: thread i mod 256 of 256
 *     adds dR[i] + dD[i] over its cells in ascending i, and the 256 sums are folded by halves (k += k + 128, k + 64, ..); the order
 *     depends on F alone.  It passes that to the attaining cell with the lowest flat index t 21 + b, clean before degraded at the
 *     same index; from there it goes on through that cell's floors as above.
 *   Map: with g the call's upstream value for the row, every map cell receives gm = g / (21 F).  Per cell, with l and s the map's
 *     two factors, Dl = mu_R^2 + mu_D^2 + C1, Ds = sigma_R sigma_D + C3: d cov = gm l / Ds; d (sigma_R sigma_D) = -(gm l s) / Ds;
 *     d var_R = d (sigma_R sigma_D) sigma_D / (2 sigma_R) where var_R > 0, else 0 (var_D alike); d mu_R = gm s (2 mu_D - 2 l mu_R) /
 *     Dl - d cov mu_D - 2 d var_R mu_R (mu_D alike); d w*R^2 = d var_R, d w*D^2 = d var_D, d w*(R D) = d cov.
 *   Window: the 3 x 3 window's adjoint honours the replicated edges: cell (t, b) receives w[dt][db] (d mu + 2 X d w*X^2 + Y d w*(XY))
 *     of every map cell (t', b') and window offset (dt, db) whose clamped index (clamp(t' + dt), clamp(b' + db)) lands on it - nine
 *     terms for every cell, several of them from the same map cell at an edge - added in the order t' ascending, dt ascending
 *     inside, b' ascending inside that, db ascending innermost.  X is the plane's own value at (t, b), Y the other plane's.
 *   dB: d S = d X (10 / ln 10) / S where S > eps and 10 log10 S > -45, else 0.
 *   Gammatone: with y the cascade's W outputs of frame t and band b, q[n] = c y[n] with c = dS / (S W) (0 where acc == 0).  Each
 *     section from the zero state is a lower-triangular Toeplitz map whose transpose is the same section run over the time-reversed
 *     sequence, so the frame's gradient is rev(sec0(sec1(sec2(sec3(rev(q)))))) in that section order, each section in the forward's
 *     arithmetic (y = b0 x + z1; z1 = b1 x - a1 y + z2; z2 = -a2 y) from the zero state.  A sample's value: for every frame that
 *     covers it, in ascending frame order, the frame's 21 band values are added in ascending band order, and the frames' sums are
 *     added in that order; the result is rounded to fp32 once.
 *   NaN: a row whose NSIM is NaN gets NaN in every cell of its dspec, and from there NaN over the samples of its whole frames,
 *     [0, (F - 1) H + W); a NaN in dspec makes the samples of its frame NaN (silent frames included).  No other row changes a bit.
 *     Samples of a trailing partial frame, and everything from the length to the stride, are written as 0.
 *
 *   nomad_nsim_backward       spec_ref_dev, spec_deg_dev, B, G, frames_host, intensity_range as nomad_nsim took them; grad_nsim_dev
 *                             [B G] float64 -> dspec_deg_out_dev [G sum F_b][21] float64, packed as spec_deg_dev.  One workgroup
 *                             per degraded row; it rebuilds the floored planes by the forward's own steps, so every comparison
 *                             sees the forward's bits.  A row has the bits of its own B = 1, G = 1 call.
 *   nomad_gammatone_backward  x_dev, R, stride, lens_host, sample_rate as nomad_gammatone took them (4-byte alignment is all the rows
 *                             need, nothing behind a length is read); dspec_dev [sum F_r][21] float64 -> dx_out_dev [R][stride]
 *                             fp32, every element written.  A row has the bits of its own R = 1 call whatever the batch, the
 *                             stride and the base address.  The cascade's outputs are stored, not recomputed: the workspace holds
 *                             W 21 doubles per frame (csrc/nsim_bwd.hip.h).
 * Contract as the forward calls: asynchronous on the caller's stream, no allocation, deterministic, no atomics; the host tables are
 * copied into the workspace ahead of the kernels; argument errors return before anything is queued, with the forward calls' codes
 * for the same causes (NOMAD_ERR_INVALID also for a NULL grad_nsim_dev, dspec_dev or output; NOMAD_ERR_WORKSPACE).  Workspace:
 *   nomad_nsim_backward_scratch_bytes(B, G, total_frames) = nomad_nsim's two tables + 9 x 8 x 21 G total_frames bytes;
 *   nomad_gammatone_backward_scratch_bytes(R, stride, sample_rate) = nomad_gammatone's three tables + 8 x 21 W R F(stride) bytes,
 *   F(stride) = nomad_gammatone_frames(stride, sample_rate) (0 for arguments the call would refuse, a stride below one frame
 *   among them); both are written before they are read.
 */
size_t nomad_nsim_backward_scratch_bytes(int B, int G, long long total_frames);
int nomad_nsim_backward(nomad_ctx* ctx, const double* spec_ref_dev, const double* spec_deg_dev, int B, int G, const int* frames_host /* [B] */,
                        double intensity_range, const double* grad_nsim_dev /* [B G] */, double* dspec_deg_out_dev /* [G sum F_b][21] */,
                        void* ws_dev, size_t ws_bytes, nomad_stream_t stream);
size_t nomad_gammatone_backward_scratch_bytes(int R, int stride, int sample_rate);
int nomad_gammatone_backward(nomad_ctx* ctx, const float* x_dev, int R, int stride, const int* lens_host, int sample_rate,
                             const double* dspec_dev /* [sum F_r][21] */, float* dx_out_dev /* [R][stride] */, void* ws_dev, size_t ws_bytes,
                             nomad_stream_t stream);

/* ---- time alignment: the delay of every degraded row against its clean clip, and the rows moved by it ----------------------
 * A codec round trip (the reference's MP3, Opus and Vorbis conditions), a model with latency or a recording through a device shifts
 * and pads a file by hundreds to thousands of samples; nomad_nsim on such a row compares frames that do not belong together.
 * clean_dev is [B][stride] fp32, clip b in its first lens_host[b] = n_b samples; deg_dev is [B G][deg_stride] fp32, row r = b G + g
 * belongs to clip b and has its OWN length deg_lens_host[r] = m_r, which may differ from n_b.  Nothing behind a length is read
 * (anything, NaN included, may stand there); rows need 4-byte alignment only and the strides need not be multiples of 4.
 *
 * Definition.  For every integer lag d in [-D, D], D = max_delay (0 .. 16384 samples, 1.024 s at 16 kHz):
 *   c_r[d] = sum over i with 0 <= i < n_b and 0 <= i + d < m_r of x_b[i] y_r[i + d].
 * d > 0 means the degraded row is late.  A lag with no overlap gives exactly 0.
 * Arithmetic and order: fp32 products and fp32 chains on the matrix cores (v_mfma_f32_16x16x4_f32), no rounding skipped or added.
 * With t = i + 16 j, j = ((d + D) mod 256) / 16, one chain covers the terms whose t lies in one SLICE [4096 k, 4096 (k + 1)), t
 * ascending; the slices of a lag are then added in float64 in ascending order - eight at a time inside a workgroup, then the
 * groups of eight, again ascending, by a second launch without atomics.  Products with a padding zero are formed and add +-0.  The
 * order depends on (n_b, m_r, D) and the lag alone: row r of any batch has the bits of its own B = 1, G = 1 call, whatever the
 * strides and the base alignment.  Integer-valued inputs whose sums stay below 2^24 per slice give the exact sums; otherwise
 *   |c - exact| <= (4096 + 8) 2^-24 sum |x_b[i]| |y_r[i + d]|   (the running-error bound of the chains; underflow aside).
 * Selection: delay_out_dev[r] is the lag of the largest c_r[d] - the sign counts, there is no normalisation by the overlap -,
 * ties going to the smaller |d|, then to the non-negative lag; peak_out_dev[r] is that c_r[d].  A silent row ties everywhere and gets
 * 0.  If any c_r[d] is NaN the delay is 0 and the peak NaN.  corr_out_dev, if not NULL, receives every c_r[d] as [B G][2 D + 1]
 * float64, lag -D first; delay and peak keep their bits without it.
 * Non-finite samples: a NaN sample that some lag reaches makes c_r NaN there (and, against padding zeros, at up to 255 further
 * lags), so the row's (for a clean clip: its G rows') delay is 0 and its peak NaN; an infinite sample does the same wherever it
 * meets a zero - a padding zero included (0 x inf) - or an infinity of the other sign.  No other row changes a bit.
 *
 *   nomad_align_shift   out[r][i] = y_r[i + delay_dev[r]] for 0 <= i < out_lens_host[r] and 0 <= i + delay_dev[r] < m_r, 0 otherwise and
 *                       from out_lens_host[r] to out_stride; R rows of deg_stride, out_dev [R][out_stride].  delay_dev is read from
 *                       DEVICE memory (nomad_align_delay's output, no host round trip; any int is taken).  A copy: the samples keep
 *                       their bits.  With out_lens_host[r] = n_b the result is a packed batch nomad_gammatone / nomad_embed_ragged read.
 *
 * NOT offered: sub-sample delays, a per-patch re-alignment in the time domain (nomad_nsim_patches moves patches by whole frames of
 * the spectrogram; clock drift is followed only so far), a polarity search (an inverted row finds some other lag), a gradient.  How close the delays are to those of ViSQOL's aligner has not been measured.
 * Contract as the degradations above: asynchronous on the caller's stream, no allocation, deterministic, no atomics; the host
 * tables are copied into the workspace ahead of the kernels, so the host arrays may die on return; workspace
 * nomad_align_scratch_bytes(B, G, stride, deg_stride, max_delay) bytes (0 for arguments the call would refuse; it covers a
 * nomad_align_shift of the same B G rows, which needs 2 x (4 R rounded up to 256) bytes), written before it is read.  Argument
 * errors return before anything is queued.
 * NOMAD_ERR_INVALID: a NULL pointer other than corr_out_dev, B outside 1 .. 65535 (R outside 1 .. 65535 x 64), G outside 1 .. 64,
 * max_delay outside 0 .. 16384, a length below 1, a stride shorter than a length (or above 2^30).  NOMAD_ERR_WORKSPACE: ws_bytes too
 * small.
 */
size_t nomad_align_scratch_bytes(int B, int G, int stride, int deg_stride, int max_delay);
int nomad_align_delay(nomad_ctx* ctx, const float* clean_dev, int B, int stride, const int* lens_host, const float* deg_dev, int G,
                      int deg_stride, const int* deg_lens_host /* [B G] */, int max_delay, int* delay_out_dev /* [B G] */,
                      double* peak_out_dev /* [B G] */, double* corr_out_dev /* [B G][2 max_delay + 1] or NULL */, void* ws_dev,
                      size_t ws_bytes, nomad_stream_t stream);
int nomad_align_shift(nomad_ctx* ctx, const float* deg_dev, int R, int deg_stride, const int* deg_lens_host, const int* delay_dev,
                      const int* out_lens_host, float* out_dev, int out_stride, void* ws_dev, size_t ws_bytes, nomad_stream_t stream);

/* ---- patch-wise NSIM: a voice-activity gate on the clean clip and a search for every patch in the degraded row --------------
 * nomad_nsim lays ONE map over the whole clip: a row whose delay changes inside the file (dropped or inserted frames, a device
 * with its own clock, a concatenating model) gets a number that is too low, and silence counts like speech.  nomad_nsim_patches
 * cuts the clean spectrogram into patches, keeps the active ones, finds for each where it best sits in the degraded spectrogram
 * and averages the patches' similarities.
 *
 * WHAT THIS IS NOT: a port of ViSQOL.  Like the measure it extends it is modelled on what ViSQOL's speech mode is remembered to do;
 * the text below is the definition, tests/patch_nsim_ref.py restates it, and its agreement with the ViSQOL binary has never been
 * measured.  NOT offered: a time-domain fine alignment per patch, sub-sample delays, a polarity search, a MOS mapping, a gradient.
 *
 * Inputs, both from nomad_gammatone: spec_ref_dev [sum F_b][21] (B clean clips, F_b = frames_host[b]) and spec_deg_dev
 * [sum over rows Fd_r][21]: degraded row r = b G + g belongs to clip b and has its OWN frame count Fd_r = deg_frames_host[r], shorter
 * or longer than F_b, rows packed in that order; no nomad_align_shift has to come first.  Everything is float64.
 * Parameters: patch in 1 .. 64 frames, search in 0 .. 128 frames, vad_ratio in (0, 1], min_active_frames in 1 .. patch,
 *   intensity_range as in nomad_nsim.
 * Activity, per clean clip: E_t = sum_b S[t][b]^2, bands ascending from 0, each product rounded and then added (no fused
 *   multiply-add).  Frame t is active iff E_t >= vad_ratio * max_t E_t, the product rounded once, the maximum formed so that a NaN
 *   sticks.  A silent clip is active everywhere (0 >= 0).
 * Patches: clip b has P_b = F_b / patch patches (integer division; nomad_nsim_patch_count(F_b, patch)); patch p covers the clean
 *   frames [s, s + patch) with s = p patch, trailing frames are in none.  Its candidate window in row r is
 *   [lo, hi] = [max(s - search, 0), min(s + search, Fd_r - patch)].  The patch is KEPT for row r iff at least min_active_frames
 *   of its frames are active and lo <= hi.
 * Candidates: q_p[u] for u in [lo, hi] is nomad_nsim of the cut-out pair spec_ref[s .. s + patch) and spec_deg_r[u .. u + patch),
 *   taken as two spectrograms of `patch` frames exactly as that call defines it: dB and absolute floor, the per-frame peak floor
 *   over both, the minimum over both subtracted, the 3 x 3 window with its edges replicated at the PATCH's own edges, the
 *   sequential band means, the mean of 21.  A candidate and its 21 band values have the BITS of a nomad_nsim call (B = 1, G = 1,
 *   frames = patch) on the cut-outs.
 * Selection, over the kept patches k = 0 .. K - 1 of a row in patch order (starts s_k, windows [lo_k, hi_k]): T_0[u] = q_0[u];
 *   T_k[u] = T_{k-1}[a_k(u)] + q_k[u], where a_k(u) is the best u' in [lo_{k-1}, min(u, hi_{k-1})] under the order: larger T, then
 *   smaller |u' - s_{k-1}|, then smaller u'.  The places of a chain so never decrease; lo_k and hi_k do not decrease in k, so
 *   a chain always exists.  The row's chain ends at the best u of the last window under the same order and is traced back through a.
 * Results per row: nsim = T_best / K; bands[j] = the chosen candidates' band values j added in ascending k, divided by K;
 *   offsets[p] = u_p, the chosen place of patch p, -1 for a patch that is not kept; patch_nsim[p] = q_p[u_p], NaN where not kept.
 *   K = 0 (a clip or a row shorter than a patch, nothing active enough) gives NaN, all offsets -1.  A silent pair gives exactly 1.
 * Non-finite values: a NaN anywhere in a clean clip's spectrogram voids its G rows; a row one of whose candidates is NaN - a NaN
 *   in a degraded frame inside some kept patch's window [lo, hi + patch) makes one - is void too: NaN results, offsets -1.  A NaN
 *   outside every window is not seen.  No other row changes a bit.
 *
 *   nomad_nsim_patches  -> nsim_out_dev [B G]; bands_out_dev [B G][21], offsets_out_dev [B G][out_patches] int32, patch_nsim_out_dev
 *                       [B G][out_patches], cand_out_dev [B G][out_patches][2 search + 1], each or NULL; out_patches >= every P_b and
 *                       >= 1, entries from P_b on are -1 / NaN.  cand_out_dev receives every q_p[u] at column u - (s - search), NaN
 *                       where there is no candidate (for a void row too).  The other outputs keep their bits with or without
 *                       any optional output, and a row has the bits of its own B = 1, G = 1 call.  Three launches: the activity
 *                       per clean clip, the candidates (one workgroup per row and patch; csrc/nsim_patches.hip.h states the
 *                       layout), the selection per row.
 * Contract as nomad_nsim: asynchronous on the caller's stream, no allocation, deterministic, no atomics; both host tables are
 * copied into the workspace ahead of the kernels, so they may die on return; workspace nomad_nsim_patches_scratch_bytes(B, G,
 * total_ref_frames = sum F_b, total_deg_frames = sum Fd_r, patch, search) bytes (0 for arguments the call would refuse), written
 * before it is read.  Argument errors return before anything is queued.
 * NOMAD_ERR_INVALID: a NULL context, spectrogram, table, nsim_out_dev or workspace; B outside 1 .. 65535, G outside 1 .. 64, patch
 * outside 1 .. 64, search outside 0 .. 128, vad_ratio outside (0, 1] (a NaN included), min_active_frames outside 1 .. patch, an
 * intensity range that is not finite and positive, a frame count below 1, out_patches below 1 or below a clip's P_b, more than
 * 2^31 - 1 (row, patch) workgroups.  NOMAD_ERR_WORKSPACE: ws_bytes too small.
 */
int nomad_nsim_patch_count(int frames, int patch);
size_t nomad_nsim_patches_scratch_bytes(int B, int G, long long total_ref_frames, long long total_deg_frames, int patch, int search);
int nomad_nsim_patches(nomad_ctx* ctx, const double* spec_ref_dev, const double* spec_deg_dev, int B, int G,
                       const int* frames_host /* [B] */, const int* deg_frames_host /* [B G] */, int patch, int search, double vad_ratio,
                       int min_active_frames, double intensity_range, int out_patches /* >= every P_b, >= 1 */,
                       double* nsim_out_dev /* [B G] */, double* bands_out_dev /* [B G][21] or NULL */,
                       int* offsets_out_dev /* [B G][out_patches] or NULL */, double* patch_nsim_out_dev /* [B G][out_patches] or NULL */,
                       double* cand_out_dev /* [B G][out_patches][2 search + 1] or NULL */, void* ws_dev, size_t ws_bytes,
                       nomad_stream_t stream);

/* ---- bf16 path (BASELINE config C5: long-form clips) ---------------------------------------- */
/*
 * The reference is fp32 only (torch 1.12, no AMP); this path exists for throughput on long clips.
 * Activations and weights are bf16 in HBM, every accumulation, bias/GELU/residual, GroupNorm/LayerNorm
 * statistic and the attention softmax are fp32.  Accuracy is reported against this library's fp32 path.
 *   nomad_enable_bf16          builds the bf16 weight copies once (allocates)
 *   nomad_embed_bf16           scoring forward: wav [B][n_samples] fp32 -> emb [B][256] fp32
 *   nomad_workspace_bytes_bf16 scratch size for it
 */
int nomad_enable_bf16(nomad_ctx* ctx);
int nomad_workspace_bytes_bf16(const nomad_ctx* ctx, int B, int n_samples, size_t* bytes);
int nomad_embed_bf16(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, float* emb_dev,
                     void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
/* bf16 counterpart of nomad_embed_ragged (files of different lengths, e.g. long-form recordings through predict):
 * same arguments, no head override; every clip's result equals its own single-clip nomad_embed_bf16 call */
int nomad_workspace_bytes_ragged_bf16(const nomad_ctx* ctx, int B, const int* lengths_host, size_t* bytes);
int nomad_embed_ragged_bf16(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                            float* emb_dev, void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);

/* ---- bf16x3: fp32-class scoring on the bf16 matrix cores -------------------------------------
 * Same surface as nomad_embed (TripletModel.forward, nomad.py:224-231), for callers who want the reference's
 * scores to its stated tolerance (1e-4) at more than the fp32 MFMA rate.  Every GEMM operand is kept as two bf16
 * planes, hi = bf16(x) and lo = bf16(x - hi) (16 mantissa bits, the bytes of one fp32), and multiplied as three
 * bf16 MFMA products hi*hi + hi*lo + lo*hi with fp32 accumulation - the conv stack, every dense layer, the grouped
 * pos-conv (as a Toeplitz GEMM over 5-frame blocks) and both attention products; bias, GELU, residuals, LayerNorm,
 * softmax and the head are fp32.  Accuracy is measured against the fp32 path in tests/test_gpu_bf16x3.py
 * (NOMAD scores agree to ~1e-6).  Forward only: no backward (the branch of nomad.forward() that carries the gradient
 * stays on nomad_embed_train).
 *   nomad_enable_bf16x3          builds the split weight copies (allocates once; call again after nomad_train_* /
 *                                weight updates)
 *   nomad_embed_bf16x3           wav [B][n_samples] fp32 -> emb [B][256] fp32
 *   nomad_workspace_bytes_bf16x3 scratch size for it
 */
int nomad_enable_bf16x3(nomad_ctx* ctx);
int nomad_workspace_bytes_bf16x3(const nomad_ctx* ctx, int B, int n_samples, size_t* bytes);
int nomad_embed_bf16x3(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, float* emb_dev,
                       void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);
/* LossNetLayers.forward (nomad.py:243-258) on the bf16x3 path - what the no-gradient `clean` branch of nomad.forward()
 * runs on: like nomad_embed with layers_out, i.e. optional head override (both or neither), emb [B][256] and
 * layers_out [12][B*T][768] fp32 (the fp32 LayerNorm output of every encoder layer).  Same workspace as
 * nomad_embed_bf16x3. */
int nomad_embed_layers_bf16x3(nomad_ctx* ctx, const float* wav_dev, int B, int n_samples, const float* head_w_dev,
                              const float* head_b_dev, float* emb_dev, float* layers_out_dev, void* workspace_dev,
                              size_t workspace_bytes, nomad_stream_t stream);
/* bf16x3 counterpart of nomad_embed_ragged (files of different lengths in one launch sequence - what predict uses):
 * same arguments, no head override; every clip's result equals its own single-clip nomad_embed_bf16x3 call */
int nomad_workspace_bytes_ragged_bf16x3(const nomad_ctx* ctx, int B, const int* lengths_host, size_t* bytes);
int nomad_embed_ragged_bf16x3(nomad_ctx* ctx, const float* wav_dev, int B, int stride, const int* lengths_host,
                              float* emb_dev, void* workspace_dev, size_t workspace_bytes, nomad_stream_t stream);

/* ---- WAV front end of the file-scoring loop (host only, no GPU work) ------------------------
 * Nomad.get_embeddings_csv (nomad.py:171-183) calls load_processing (nomad.py:192-212) per file:
 * torchaudio.load -> fp32 in [-1, 1), mean of the first two channels, resample to 16 kHz.  These two
 * entry points do the first two steps on plain host threads, straight into the rows of the (pinned)
 * staging buffer nomad_embed_ragged* reads after one H2D copy; nomad_wav_read_rows also resamples.
 * Decoded: PCM 8/16/24/32 (x 2^-(bits-1)), IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE of those. */
typedef struct nomad_wav_info {
    int sample_rate, channels, format_tag, bits;
    long long frames;      /* per channel; a data chunk cut short by the end of the file counts what is there */
    long long data_offset; /* byte offset of the sample data */
} nomad_wav_info;
/* Headers of n files on `threads` host threads.  status[i] = NOMAD_OK, NOMAD_ERR_IO or NOMAD_ERR_FORMAT per
 * file (info[i] zeroed then); the return value is NOMAD_OK unless the arguments are bad. */
int nomad_wav_probe(const char* const* paths, int n, nomad_wav_info* info, int* status, int threads);
/* Frames a probed file has at target_rate: its own count, or ceil(frames * target / rate) after resampling. */
int nomad_wav_frames_at(const nomad_wav_info* info, int target_rate, long long* frames);
/* Sample data of n probed files -> dst[row[i] * stride + 0 .. frames_at(info[i], target_rate)) as mono fp32 at target_rate
 * (row == NULL: row[i] = i); the rest of a row is left untouched.  A file at another rate is resampled like
 * torchaudio.transforms.Resample(rate, target_rate) with its defaults (Hann-windowed sinc, lowpass_filter_width 6, rolloff
 * 0.99; nomad.py:203-205).  Needs frames_at <= stride.  status as above; returns the first non-zero status (all files are
 * attempted). */
int nomad_wav_read_rows(const char* const* paths, const nomad_wav_info* info, int n, const int* row,
                        float* dst_host, long long stride, int target_rate, int* status, int threads);

/* ---- measurement ------------------------------------------------------------------------- */
/* Kernel classes for the in-library HIP-event timers. */
enum {
    NOMAD_K_GEMM = 0,       /* every GEMM launch (all instantiations) */
    NOMAD_K_ATTN = 1,
    NOMAD_K_FRONT = 2,
    NOMAD_K_ROW = 3,
    NOMAD_K_PAIR = 4,
    NOMAD_K_GEMM_BIG = 5,   /* of which: the 256x128 instantiation (gemm_*_glds_kernel<256,128,...>; bf16: 128x128 / 256x256) */
    NOMAD_K_GEMM_FINE = 6,  /* of which: the finer instantiations (128x128x32, 128x64x32, N = 48) */
    NOMAD_K_COUNT = 7
};
/* When enabled every kernel launch of nomad_embed/nomad_pairwise is bracketed by hipEvents on the
 * launch stream.  nomad_profile_read synchronises those events and returns, per class, the summed
 * device time (ms), launch count and algorithmic FLOPs (2*M*N*K of the true problem, no padding)
 * since the last nomad_profile_reset. */
int nomad_profile_enable(nomad_ctx* ctx, int on);
int nomad_profile_reset(nomad_ctx* ctx);
int nomad_profile_read(nomad_ctx* ctx, double ms[NOMAD_K_COUNT], long long launches[NOMAD_K_COUNT],
                       double flops[NOMAD_K_COUNT]);

/* ---- kernel-level diagnostics (used by tests/ to localise a parity failure) --------------- */
/* C[M][N] = epilogue(A[M][K] * W[N][K]^T): + bias[N] (nullable), GELU if gelu!=0, + R[M][N] (nullable).
 * tile selects the kernel instantiation.  libnomad_hip.so holds the ones the forward / backward select: 33 = 256x128x16
 * (3-stage LDS-DMA), 31 = 128x128x32, 20 = 128x128x32 (4 waves), 34 = 128x64x32, 37 = 64x64x32, 48 = N = 48 (pos-conv).
 * Every other id (register-staged kernels, ablations, A/B variants) exists in libnomad_diag.so only - the same source
 * built with -DNOMAD_DIAG for the measurement tools and kernel tests - and returns NOMAD_ERR_INVALID here. */
int nomad_diag_gemm(nomad_ctx* ctx, const float* A_dev, const float* W_dev, const float* bias_dev,
                    const float* R_dev, float* C_dev, int M, int N, int K, int gelu, int tile,
                    nomad_stream_t stream);
/* The fp32 positional convolution alone, in the frequency domain (512-point transforms, one 48 x 48 complex product per bin and
 * group), on the caller's operands.  x: the padded group-major input [16][sum_c (T_c + 128)][48] (zero frames 0..63 and
 * T_c + 64.. of every clip); v: weights [16][64][6144] ([out][tap * 48 + in], rows 48..63 unused); bias: [768] or null;
 * y = x + gelu(u), u (nullable) = pos_conv(x) + bias: [sum_c T_c][768].  lens_host: the clips' frame counts T_c.  ragged = 0:
 * the uniform launch (every T_c equal), 1: the ragged one.  Synchronous.  (libnomad_diag.so has the same hook for the direct and
 * nested F(2,2) forms under another name.) */
int nomad_diag_posconv_fft(nomad_ctx* ctx, const float* x_dev, const float* v_dev, const float* bias_dev, float* y_dev,
                           float* u_dev, int B, const int* lens_host, int ragged, nomad_stream_t stream);
/* The bf16 GEMM: A [M][K], W [N][K], R, C [M][N] are bf16; bias fp32.  tile (libnomad_hip.so): 1 = 128x128,
 * 2 = 128x64, 3 = 256x256, 4 = 64x64 (all BK = 64), 16 = 256x256 deep-pipelined; others: libnomad_diag.so. */
int nomad_diag_gemm_bf16(nomad_ctx* ctx, const void* A_dev, const void* W_dev, const float* bias_dev,
                         const void* R_dev, void* C_dev, int M, int N, int K, int gelu, int tile,
                         nomad_stream_t stream);
/* bf16x3 pieces.  nomad_diag_split_bf16: fp32 in[n] -> split planes out (hi at 0, lo at `plane` bf16 elements), or back
 * (inverse != 0: `in` is the split buffer, `out` fp32).  nomad_diag_gemm_bf16x3: the split GEMM on split A [M][K]
 * (planes M*K apart), W [N][K] (N*K apart), optional R [M][N] (M*N apart); C is split (M*N apart) or fp32 (out_f32). */
int nomad_diag_split_bf16(nomad_ctx* ctx, const float* in_dev, void* out_dev, long long plane, long long n, int inverse,
                          nomad_stream_t stream);
int nomad_diag_gemm_bf16x3(nomad_ctx* ctx, const void* A_dev, const void* W_dev, const float* bias_dev,
                           const void* R_dev, void* C_dev, int M, int N, int K, int gelu, int out_f32,
                           nomad_stream_t stream);
/* bf16x3 attention: split qkv [B*T][2304] (planes B*T*2304 apart, q pre-scaled) -> split out [B*T][768].
 * waves: -1 = what the forward uses, 0 = the tiled kernel, 4 / 8 = the K/V-resident kernel (T <= 256) with that many
 * waves per (clip, head). */
int nomad_diag_attention_bf16x3(nomad_ctx* ctx, const void* qkv_dev, void* out_dev, int B, int T, int waves,
                                nomad_stream_t stream);
/* bf16 attention: qkv [B*T][2304] bf16 (q pre-scaled by 64^-0.5) -> out [B*T][768] bf16.  q_has_log2e must be != 0: q is
 * additionally scaled by log2(e), as the bf16 forward's QKV projection produces it (the kernel works in log2 units);
 * 0 (plain q, scaled inside the kernel) is NOMAD_ERR_INVALID: that kernel went with round 5's move to 16x16x32. */
int nomad_diag_attention_bf16(nomad_ctx* ctx, const void* qkv_dev, void* out_dev, int B, int T, int q_has_log2e,
                              nomad_stream_t stream);
/* out[M][N] = LayerNorm(in[M][N]) * gamma + beta, N in {512, 768}, eps 1e-5. */
/* one wave spins for spin_ticks of the 100 MHz wall counter; out_dev[0] = shader-clock cycles elapsed, out_dev[1] = wall
 * ticks: run it on a second stream to read the clock a kernel under test actually gets */
int nomad_diag_clock_probe(nomad_ctx* ctx, unsigned long long spin_ticks, unsigned long long* out_dev,
                           nomad_stream_t stream);
int nomad_diag_layernorm(nomad_ctx* ctx, const float* in_dev, const float* gamma_dev, const float* beta_dev,
                         float* out_dev, int M, int N, nomad_stream_t stream);
/* ctx_out[B*T][768] = softmax(q k^T) v per head, from qkv[B*T][2304] (q pre-scaled). */
int nomad_diag_attention(nomad_ctx* ctx, const float* qkv_dev, float* out_dev, int B, int T, nomad_stream_t stream);
/* dx[M][N] = LayerNorm backward of g w.r.t. the LN input x (weights frozen). */
int nomad_diag_layernorm_bwd(nomad_ctx* ctx, const float* x_dev, const float* g_dev, const float* gamma_dev,
                             float* dx_dev, int M, int N, nomad_stream_t stream);
/* Runs the attention forward (ctx_out [B*T][768], lse [B*12][T]) then its backward: dqkv [B*T][2304]. */
int nomad_diag_attention_bwd(nomad_ctx* ctx, const float* qkv_dev, const float* dctx_dev, float* ctx_out_dev,
                             float* lse_dev, float* dqkv_dev, int B, int T, nomad_stream_t stream);
/* With on!=0 every conv layer output gets its own workspace region (no ping-pong aliasing), so
 * nomad_diag_workspace_region can read all of them back after nomad_embed.  Changes
 * nomad_workspace_bytes. */
int nomad_diag_keep_intermediates(nomad_ctx* ctx, int on);
/* Byte offset and size of a named intermediate inside the nomad_embed workspace for (B, n_samples):
 * "conv0".."conv6" (time-major [B][L_i][512]), "featln" [B*T][512], "xpad" [16 groups][B][T+128][48]
 * (post_extract_proj output, group-major, at frames 64..64+T of each clip; zero frames around). */
int nomad_diag_workspace_region(const nomad_ctx* ctx, int B, int n_samples, const char* name,
                                size_t* offset, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* NOMAD_HIP_H */
