/*
 * qpd.h -- C-ABI of the MI355X quantized polar decoder (libqpd.so).
 *
 * The drop-in boundary for the reference's L1 decoders.  Each entry point
 * replaces one piece of the reference's pybind11 surface
 * (/root/reference/PolarDecoder/PolarDecoder/_cpp):
 *
 *   qpd_create    <- the decoder constructors, which copy every table into the
 *                    object:  SCLUT::SCLUT        src/SCLUTDecoder.cpp:10-19
 *                             SCLLUT::SCLLUT      src/SCLLUTDecoder.cpp:33-44
 *                             FastSCLUT::FastSCLUT src/FastSCLUT.cpp:13-24
 *                             FastSCLLUT::FastSCLLUT src/FastSCLLUTDecoder.cpp:42-55
 *                             SC::SC              src/SCDecoder.cpp:7-12
 *                             CASCLLUT::CASCLLUT  src/CASCLLUTDecoder.cpp:43-62
 *                             CAFastSCLLUT::CAFastSCLLUT src/CAFastSCLLUTDecoder.cpp:43-56
 *                             SCL::SCL            src/SCLDecoder.cpp:30-36
 *                             CASCL::CASCL        src/CASCLDecoder.cpp:42-54
 *                             FastSC::FastSC      src/FastSCDecoder.cpp:13-19
 *                             FastSCL::FastSCL    src/FastSCLDecoder.cpp:40-47
 *                             SCUniformQuantizedDecoder  src/SCUniformQuantizedDecoder.cpp:9-18
 *                             SCLUniformQuantizedDecoder src/SCLUniformQuantizedDecoder.cpp:31-41
 *                             SCLloydQuantizedDecoder    src/SCLloydQuantizedDecoder.cpp:6-20
 *                             SCLLloydQuantizedDecoder   src/SCLLloydQuantizedDecoder.cpp:29-44
 *                   bound at py_interface/py_*.cpp (all 15 classes of
 *                   _libPolarDecoder.cpp:29-50)
 *   qpd_decode    <- SCLUT::decode   src/SCLUTDecoder.cpp:21-124
 *                    SCLLUT::decode  src/SCLLUTDecoder.cpp:47-253
 *                    FastSCLUT::decode src/FastSCLUT.cpp:27-206
 *                    FastSCLLUT::decode src/FastSCLLUTDecoder.cpp:57-408
 *                    CASCLLUT::decode src/CASCLLUTDecoder.cpp:64-303
 *                    CAFastSCLLUT::decode src/CAFastSCLLUTDecoder.cpp:58-454
 *                   (batched: B frames per call instead of one)
 *   qpd_decode_f64 <- SC::decode     src/SCDecoder.cpp:14-89 (float64 LLR input)
 *                    SCL::decode    src/SCLDecoder.cpp:38-176
 *                    CASCL::decode  src/CASCLDecoder.cpp:74-249
 *                    FastSC::decode src/FastSCDecoder.cpp:21-174
 *                    FastSCL::decode src/FastSCLDecoder.cpp:49-423
 *                    SC{,L}UniformQuantizedDecoder::decode src/SCUniformQuantizedDecoder.cpp:20-99,
 *                        src/SCLUniformQuantizedDecoder.cpp:43-184
 *                    SC{l,L}loydQuantizedDecoder::decode src/SCLloydQuantizedDecoder.cpp:22-101,
 *                        src/SCLLloydQuantizedDecoder.cpp:46-187
 *   qpd_decode_u8 / qpd_decode_u8_host: qpd_decode / qpd_decode_host from uint8
 *                   symbols (no reference counterpart: its array_t<int> is int32)
 *   qpd_decode_host / qpd_decode_f64_host: the same from host buffers
 *                   (copy in, decode, copy out, synchronous) -- what a
 *                   per-frame `decode(symbols)` call needs.
 *   qpd_destroy   <- the pybind11 object's destructor
 *
 * Plain pointers and sizes only; no torch or HIP types in the signatures
 * (streams are passed as `void*` = hipStream_t, NULL = default stream).
 *
 * Errors: every function returns QPD_OK (0) or a negative QPD_E* code and
 * records a message retrievable with qpd_last_error() (thread-local).  The
 * reference performs no validation (out-of-range symbols are UB there); this
 * library rejects bad configurations at create time and flags out-of-range
 * channel symbols on the device (reported by the host entry points and by
 * qpd_check_input_error()).
 */
#ifndef QPD_H
#define QPD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPD_ABI_VERSION 7

/* Decoder kinds (the reference's class names). */
enum qpd_kind {
    QPD_SC_FLOAT = 0,    /* SCDecoder       (min-sum on float64 LLRs)        */
    QPD_SC_LUT = 1,      /* SCLUTDecoder                                      */
    QPD_SCL_LUT = 2,     /* SCLLUTDecoder                                     */
    QPD_FASTSC_LUT = 3,  /* FastSCLUTDecoder  (R0/R1/REP/SPC shortcuts)       */
    QPD_FASTSCL_LUT = 4, /* FastSCLLUTDecoder (R0/R1/REP shortcuts; no SPC)   */
    QPD_CASCL_LUT = 5,   /* CASCLLUTDecoder     (SCL-LUT + CRC-aided output)   */
    QPD_CAFASTSCL_LUT = 6, /* CAFastSCLLUTDecoder (FastSCL-LUT + CRC-aided output) */
    /* float64-LLR decoders (qpd_decode_f64) */
    QPD_SCL_FLOAT = 7,   /* SCLDecoder        (min-sum list; PM init 1e300)    */
    QPD_CASCL_FLOAT = 8, /* CASCLDecoder      (SCL + CRC from crc_n/crc_loc)   */
    QPD_FASTSC_FLOAT = 9,   /* FastSCDecoder  (R0/R1/REP/SPC shortcuts)        */
    QPD_FASTSCL_FLOAT = 10, /* FastSCLDecoder (R0/R1/REP shortcuts; no SPC)    */
    QPD_SC_UNIFORM = 11,  /* SCUniformQuantizedDecoder  (Q after every f/g)   */
    QPD_SCL_UNIFORM = 12, /* SCLUniformQuantizedDecoder                       */
    QPD_SC_LLOYD = 13,    /* SCLloydQuantizedDecoder    (bisect after f/g)    */
    QPD_SCL_LLOYD = 14    /* SCLLloydQuantizedDecoder                         */
};

enum qpd_status {
    QPD_OK = 0,
    QPD_E_INVALID = -1,     /* bad argument / configuration                  */
    QPD_E_UNSUPPORTED = -2, /* valid for the reference, not supported here -- or
                             * not by the engine asked for (QPD_ENGINE_FAST on
                             * tables, a list size or a plan it does not serve:
                             * qpd_last_error() says which)                  */
    QPD_E_DEVICE = -3,      /* HIP runtime failure                           */
    QPD_E_INPUT = -4        /* input the reference cannot decode defined-ly,
                               seen on device: a channel symbol outside
                               [0, v); a Lloyd index outside the
                               reconstruction list; a NaN path metric; a NaN
                               LLR given to the channel quantizer           */
};

/*
 * Decoder description.  All arrays are host pointers, copied at create time
 * (the reference's ctors copy too).
 *
 * Tables use the packed layout (quantized_decoder_polar_codes_amd/lut.py):
 *   f table t : lut_f[t*v*v + a*v + b]              a = first-half symbol
 *   g table t : lut_g[(t*2 + u)*v*v + a*v + b]      u = left partial sum
 *   node p = 2^depth + node - 1, element j of that node uses table
 *            f_base[p] + j*f_step  (f_step = 0: one table per node)
 *   vcl[((row*N) + pos)*v + sym], row in [0, vcl_rows)
 */
typedef struct qpd_config {
    int32_t kind;               /* enum qpd_kind                                  */
    int32_t N;                  /* code length, power of two, 2..65536            */
    int32_t K;                  /* output bits = number of 0 entries in frozen    */
    int32_t L;                  /* list size (SCL kinds), 1..32; ignored otherwise.  Fast engine: L <= 8;
                                 * SCL-LUT / CA-SCL-LUT also 9..16; FastSCL-LUT / CA-FastSCL-LUT 9..16 only on
                                 * an explicit QPD_ENGINE_FAST (AUTO: generic engine).  Above: generic engine */
    int32_t v;                  /* symbol alphabet size, 2..256 (LUT kinds); the
                                   re-quantizer's v (uniform kinds: M = (v/2 - 0.5) r_f,
                                   (v/2 - 1) r_g, integer v/2)                    */
    const int32_t *frozen_bits; /* [N], 1 = frozen, 0 = information               */
    const int32_t *node_type;   /* [2N-1] node labels (Fast kinds), else NULL     */
    const uint8_t *lut_f;       /* [lut_f_count][v][v]                            */
    int32_t lut_f_count;
    const int32_t *f_base;      /* [N-1]                                          */
    int32_t f_step;             /* 0 or 1                                         */
    const uint8_t *lut_g;       /* [lut_g_count][2][v][v]                         */
    int32_t lut_g_count;
    const int32_t *g_base;      /* [N-1]                                          */
    int32_t g_step;             /* 0 or 1                                         */
    const double *vcl;          /* [vcl_rows][N][v], finite                       */
    int32_t vcl_rows;           /* >= log2(N)                                     */
    int32_t device;             /* HIP device ordinal (-1 = current device)       */
    int32_t max_waves;          /* persistent-grid size cap (0 = default)         */
    int32_t engine;             /* enum qpd_engine (0 = auto)                     */
    /* CRC-aided kinds only (ignored otherwise).  Output = the first A info bits
     * of the first path, in stable path-metric order, whose info bits [0, A)
     * reproduce bits [A, K) under the CRC (CRC::encoding, utils.cpp:77-92;
     * coefficient j of the divisor is 1 for j in crc_loc).  The reference's CA
     * decoders always check CRC-24 with loc {24,23,21,20,17,15,13,12,8,4,2,1,0}
     * (CASCLLUTDecoder.h:33-34) whatever crc_n/crc_p their ctor received; the
     * Python shim passes exactly that.  Requires 1 <= A <= K, K - A <= crc_n. */
    int32_t A;                  /* message bits before the CRC                    */
    int32_t crc_n;              /* CRC length, 1..32                              */
    const int32_t *crc_loc;     /* [crc_loc_count] coefficient indices in [0, crc_n] */
    int32_t crc_loc_count;
    /* QPD_CASCL_FLOAT honours crc_n/crc_loc as given (CASCLDecoder.cpp:49-53)
     * and compares exactly crc_n bits after the A info bits: requires
     * 1 <= A, A + crc_n <= K. */
    /* Uniform kinds: step r per node_posi (decoder_r_f / decoder_r_g). */
    const double *r_f;          /* [N-1] */
    const double *r_g;          /* [N-1] */
    /* Lloyd kinds: table t (0 = f, 1 = g) of node p is
     * q_bnd[bnd_off[t*(N-1)+p] ... + bnd_len[...]) (boundaries) and
     * q_rec[rec_off[...] ... + rec_len[...]) (reconstruction values). */
    const double *q_bnd;
    int32_t q_bnd_count;
    const double *q_rec;
    int32_t q_rec_count;
    const int32_t *bnd_off;     /* [2*(N-1)] */
    const int32_t *bnd_len;     /* [2*(N-1)], >= 1 */
    const int32_t *rec_off;     /* [2*(N-1)] */
    const int32_t *rec_len;     /* [2*(N-1)], >= 1 */
} qpd_config;

/* Kernel selection.  AUTO picks FAST when the tables allow it (one table per
 * node, v <= 16) and the list size is at most 8 (SCL-LUT / CA-SCL-LUT: 16), and
 * GENERIC otherwise; the env var QPD_ENGINE overrides.  FAST asked for
 * explicitly also serves FastSCL-LUT / CA-FastSCL-LUT with 9 <= L <= 16 (lane
 * groups of 16) unless the code has an R1 node of more than 32 elements, or of
 * more than 16 whose argsort finds no room in LDS: then, as for everything else
 * the fast engine does not serve, qpd_create returns QPD_E_UNSUPPORTED. */
enum qpd_engine { QPD_ENGINE_AUTO = 0, QPD_ENGINE_GENERIC = 1, QPD_ENGINE_FAST = 2 };

typedef struct qpd_decoder qpd_decoder;

int qpd_abi_version(void);
/* Hash of the sources and flags the library was built from (build.py
 * source_hash): the Python loader refuses a library built from other sources. */
const char *qpd_build_id(void);
const char *qpd_last_error(void);

int qpd_create(const qpd_config *cfg, qpd_decoder **out);
void qpd_destroy(qpd_decoder *dec);

/* LUT kinds.  d_symbols: device int32 [B][N]; d_out: device uint8 [B][K]
 * ([B][A] for the CRC-aided kinds; qpd_info.out_bits).  Asynchronous on
 * `stream`.
 * A decoder owns its work buffers (slab, pre-pass rows, task queue, error
 * word, staging), so the library orders its calls: a call on a stream other
 * than the one the decoder's previous work ran on first makes that stream wait
 * for it (hipStreamWaitEvent), and host threads are serialized per handle.
 * Any mix of streams and host threads on one decoder therefore decodes as if
 * the calls ran one after another (the reference's synchronous contract,
 * py_SCLLUTDecoder.cpp:15); concurrent streams on ONE decoder do not overlap
 * -- use one decoder per stream for that. */
int qpd_decode(qpd_decoder *dec, const int32_t *d_symbols, int64_t B, uint8_t *d_out, void *stream);
/* The same from uint8 channel symbols (the alphabet is at most 256, and at most
 * 16 on the fast engine): d_symbols is device uint8 [B][N], a quarter of the
 * int32 input; same contract, stream ordering, range check (QPD_E_INPUT for a
 * symbol >= v) and decoded bits as qpd_decode.  A fast-engine decoder in
 * pre-mode reads the bytes as they are (the root pre-pass; fastest from an
 * 8-byte-aligned buffer); every other decoder widens them, chunk by chunk, into
 * an int32 staging buffer of its own (<= 1 GB) and runs the int32 launch
 * (qpd_info.u8_staged). */
int qpd_decode_u8(qpd_decoder *dec, const uint8_t *d_symbols, int64_t B, uint8_t *d_out, void *stream);
/* float64-LLR kinds (QPD_SC_FLOAT, 7..14).  d_llr: device float64 [B][N];
 * d_out: device uint8 [B][K] ([B][A] for QPD_CASCL_FLOAT). */
int qpd_decode_f64(qpd_decoder *dec, const double *d_llr, int64_t B, uint8_t *d_out, void *stream);

/* Host-buffer variants (synchronous) -- what the reference's per-frame
 * decode(symbols) call needs.  Small batches (qpd_info.host_max_frames; one
 * frame per call in the reference drivers) run on the host engine, a C++
 * decoder of this library for a few frames (no launch, copy or stream
 * synchronization: SCLUTDecoder.cpp:21-124 costs ~10 us per frame on one core,
 * a GPU call ~0.1 ms); larger batches on the GPU kernels.  Both decode the
 * same bits (the reference's). */
int qpd_decode_host(qpd_decoder *dec, const int32_t *h_symbols, int64_t B, uint8_t *h_out);
int qpd_decode_u8_host(qpd_decoder *dec, const uint8_t *h_symbols, int64_t B, uint8_t *h_out);
int qpd_decode_f64_host(qpd_decoder *dec, const double *h_llr, int64_t B, uint8_t *h_out);

/* Where the host-buffer calls run: AUTO (the default; the host engine up to
 * qpd_info.host_max_frames frames, the GPU above), GPU (always), CPU (the host
 * engine for every batch; QPD_E_UNSUPPORTED for the re-quantized float kinds,
 * which the host engine does not decode).  The environment variable
 * QPD_HOST_ENGINE=gpu|cpu sets it at create time. */
enum qpd_host_mode { QPD_HOST_AUTO = 0, QPD_HOST_GPU = 1, QPD_HOST_CPU = 2 };
int qpd_set_host_engine(qpd_decoder *dec, int32_t mode);

/*
 * Decode with status: what a receiver needs besides the bits of a list decode --
 * the path metric of the output path and, for the CRC-aided kinds, whether that
 * path passed the CRC -- and an optional mask on the CRC (the RNTI of PDCCH blind
 * detection).  The counterpart of the reference's float CA-SCL with RNTI,
 *     CASCL::decode(llr, RNTI) -> (bits, PM, isPass)
 *         PolarEncoder/PolarBD/_cpp/src/CASCLWithRNTI.cpp:74-252
 * (the mask at :222-224, the return value at :252; CASCLDecoder.cpp:202-234
 * computes the same PM and isPass and drops them), for every list kind here.
 *
 * in_type says what d_in holds: int32 symbols (as qpd_decode), uint8 symbols
 * (qpd_decode_u8) or float64 LLRs (qpd_decode_f64); it must fit the decoder
 * (QPD_E_INVALID otherwise).  st == NULL, or no mask and both outputs NULL:
 * exactly that call.  With crc_mask_bits == 0 the output bits are always that
 * call's.  Stream ordering, the per-handle lock, the error word and
 * qpd_info.last_engine / u8_staged as for those calls; the host variant keeps
 * their host_max_frames dispatch (qpd_set_host_engine honoured).
 *
 * metric, crc_pass: device pointers in qpd_decode_status, host pointers in
 * qpd_decode_status_host; each may be NULL.  crc_mask: always a host pointer,
 * read before the call returns.  Frames >= B are never written.
 *   metric[f]   the final path metric (the decoder's own PML double) of the path
 *               whose bits are output.  List kinds only, CRC-aided or not, on
 *               every engine; QPD_E_INVALID for the SC / FastSC kinds.
 *   crc_pass[f] CRC-aided kinds only (QPD_E_INVALID otherwise): 1 iff the output
 *               path is the first path, in argsort(PML) order, whose CRC compare
 *               succeeded (the reference's isPass; the compare is the one of
 *               qpd_config.A above: K - A bits for the LUT kinds, crc_n bits for
 *               QPD_CASCL_FLOAT); 0: none did, the output is the best-metric path.
 *   crc_mask    crc_mask_bits entries of 0 / 1; bit l is XORed onto check-code bit
 *               crc_n - crc_mask_bits + l before the compare, so it changes which
 *               path wins.  crc_mask_bits > crc_n (the reference writes out of
 *               bounds there), or any mask bits on a kind without CRC:
 *               QPD_E_INVALID.
 * A list of one path (L = 1) has no selection to report: QPD_E_UNSUPPORTED when
 * metric or crc_pass is asked for.
 * Deviation from the reference: it returns PML[i], i the winner's position in
 * the argsort order, not the winner's index (CASCLWithRNTI.cpp:234) -- the
 * winner's metric only while the final PML is ascending, which mink guarantees
 * when the code's last position is an information bit.  metric[f] here is
 * always the output path's own metric.
 */
enum qpd_input_type { QPD_IN_I32 = 0, QPD_IN_U8 = 1, QPD_IN_F64 = 2 };
typedef struct qpd_status_args {
    const uint8_t *crc_mask;   /* host, [crc_mask_bits] of 0/1, or NULL          */
    int32_t crc_mask_bits;     /* 0..crc_n                                        */
    double  *metric;           /* [B] or NULL: path metric of the output path     */
    uint8_t *crc_pass;         /* [B] or NULL: 1 = the output path passed the CRC */
} qpd_status_args;
int qpd_decode_status(qpd_decoder *dec, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                      const qpd_status_args *st, void *stream);
int qpd_decode_status_host(qpd_decoder *dec, const void *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                           const qpd_status_args *st);

/*
 * List output: all L candidates of a list decode, not only the output path -- for
 * blind detection without one decode per candidate RNTI (test any number of RNTIs
 * on the candidates' K bits; an unknown mask is CRC(info) XOR tail), for genie list
 * bounds ("was the sent word in the list?") and for re-ranking by the caller.  The
 * reference keeps these paths to the end of CASCLLUTDecoder.cpp:264-302 and drops
 * them.
 *
 * Candidate r of frame f is the path at position r of the reference's
 * argsort(PML): metric ascending, ties by list slot (the stable order libstdc++'s
 * sort gives for L <= 16) -- for every list kind, CRC-aided or not.
 *   cand_bits[f][r][t]  the path's decision at information position info_pos[t],
 *                       t < K: for the CRC-aided kinds all K bits, message and CRC
 *                       tail; for the Fast kinds after the re-encode, as the output
 *                       bits are.  Required (QPD_E_INVALID if NULL).
 *   cand_metric[f][r]   that path's own final PML double; or NULL.
 *   cand_pass[f][r]     that path's CRC compare under crc_mask (the compare of
 *                       qpd_status_args.crc_pass); CRC-aided kinds only
 *                       (QPD_E_INVALID otherwise); or NULL.
 *   chosen[f]           the r of the path whose bits d_out receives: the first
 *                       passing r for the CRC-aided kinds, else 0; or NULL.
 * d_out / h_out may be NULL; when given it receives exactly qpd_decode_status's
 * bits.  crc_mask, in_type, stream ordering, the error word and the host variant's
 * dispatch: as qpd_decode_status / _host.  The outputs are device pointers in
 * qpd_decode_list, host pointers in qpd_decode_list_host.  Frames >= B are never
 * written.
 * Refused before any launch: the SC / FastSC kinds, cand_pass or mask bits on a
 * kind without CRC, cand_bits NULL (QPD_E_INVALID); L = 1 (QPD_E_UNSUPPORTED); and
 * L > 16 (QPD_E_UNSUPPORTED): there the reference's argsort is libstdc++'s
 * unstable introsort, and the first-minimum output path of the kinds without CRC
 * need not be candidate 0.
 */
typedef struct qpd_list_args {
    const uint8_t *crc_mask;   /* host, [crc_mask_bits] of 0/1, or NULL (as qpd_status_args) */
    int32_t crc_mask_bits;     /* 0..crc_n                                                    */
    uint8_t *cand_bits;        /* [B][L][K]  required                                         */
    double  *cand_metric;      /* [B][L]     or NULL                                          */
    uint8_t *cand_pass;        /* [B][L]     or NULL; CRC-aided kinds only                    */
    int32_t *chosen;           /* [B]        or NULL                                          */
} qpd_list_args;
int qpd_decode_list(qpd_decoder *dec, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                    const qpd_list_args *ls, void *stream);
int qpd_decode_list_host(qpd_decoder *dec, const void *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                         const qpd_list_args *ls);

/*
 * Mask search: one list decode against a whole set of CRC masks -- what a PDCCH
 * receiver does for every candidate frame: it holds several RNTIs and asks which of
 * them, if any, the frame is addressed to, and on which list path.  Instead of one
 * qpd_decode_status per mask, or qpd_decode_list's L * K candidate bytes and a CRC pass
 * by the caller, every candidate is reported as one word, its CRC syndrome, and the set
 * is compared against it in the decode's tail.  CRC-aided kinds only, on every engine.
 *
 * Candidates are in qpd_decode_list's order: r = the path's position in argsort(PML)
 * (stable, L <= 16).  chk = the number of compared check bits: K - A for the LUT kinds,
 * crc_n for QPD_CASCL_FLOAT (the compare of qpd_config.A above).
 *   cand_syndrome[f][r]  bit chk-1-j = check bit j of path r (its decision at
 *                        information position A + j) XOR bit crc_n-1-j of the CRC
 *                        register after the path's A message bits, j < chk: the
 *                        compare of qpd_decode_status with no mask, collected instead
 *                        of ANDed.  0: the path passes the plain CRC.  Or NULL.
 *   cand_metric[f][r]    that path's own final PML double (qpd_list_args.cand_metric);
 *                        or NULL.
 *   crc_masks            n_masks rows of crc_mask_bits entries 0 / 1, each row placed
 *                        as qpd_status_args.crc_mask: row i has the register value
 *                        M_i = sum of crc_masks[i][l] << (crc_mask_bits - 1 - l).  Mask
 *                        i passes candidate r iff
 *                            cand_syndrome[f][r] == M_i >> (crc_n - chk)
 *                        -- exactly qpd_decode_status's compare under that mask.  With
 *                        chk == crc_n this is plain equality: a 16-bit RNTI under
 *                        which a word was sent is the syndrome itself (an unknown RNTI
 *                        is read off cand_syndrome when it is below 2^16).
 *   The output path is the lowest r that any mask passes; hit_mask[f] the lowest i that
 *   passes it (duplicate masks resolve to the first), hit_rank[f] = r.  No mask passes
 *   any candidate: hit_mask[f] = -1, hit_rank[f] = 0, the output path is the
 *   best-metric path (qpd_decode_status's "none did").  d_out receives the output
 *   path's A bits, metric[f] its own PML.  Each of the three and d_out may be NULL.
 * With n_masks == 1 the call is qpd_decode_status with that mask, bit for bit: d_out
 * and metric are its, crc_pass == (hit_mask >= 0), hit_rank == qpd_decode_list's chosen.
 * n_masks == 0: the syndromes and metrics alone; without a mask set there is no defined
 * output path, so d_out, hit_mask, hit_rank and metric must be NULL (QPD_E_INVALID).
 * crc_masks is always a host pointer, read before the call returns.  The set is kept in
 * a device buffer of the decoder's.  A call whose set equals the resident one enqueues
 * its launches and returns, as qpd_decode_list does; a call with another set first
 * uploads it on the decoder's own stream, behind the decoder's previous work (which may
 * still read the old set), and BLOCKS the host until that upload is done -- so a
 * receiver that alternates sets on one handle synchronizes once per call (use one
 * decoder per set), and such a call cannot be captured into a graph.  The outputs are
 * device pointers in qpd_decode_search, host pointers in qpd_decode_search_host.
 * Frames >= B are never written; a frame with an error flag (qpd_check_input_error)
 * keeps what the caller left.  in_type, stream ordering, the per-handle lock, the error
 * word, qpd_info.last_engine and the host variant's host_max_frames dispatch: as
 * qpd_decode_list / _host.
 * Refused before any launch: a kind without CRC, the SC / FastSC kinds, a mask entry
 * above 1, crc_mask_bits outside [0, crc_n], n_masks outside [0, QPD_MAX_SEARCH_MASKS],
 * crc_masks NULL with n_masks * crc_mask_bits > 0, an in_type that does not fit
 * (QPD_E_INVALID); L = 1 and L > 16 (QPD_E_UNSUPPORTED, as qpd_decode_list).
 */
#define QPD_MAX_SEARCH_MASKS 256
typedef struct qpd_search_args {
    const uint8_t *crc_masks;   /* host, [n_masks][crc_mask_bits] of 0/1 (each row as qpd_status_args.crc_mask) */
    int32_t n_masks;            /* 0..QPD_MAX_SEARCH_MASKS                                                      */
    int32_t crc_mask_bits;      /* 0..crc_n, one width for the whole set                                        */
    uint32_t *cand_syndrome;    /* [B][L] or NULL                                                               */
    double   *cand_metric;      /* [B][L] or NULL                                                               */
    int32_t  *hit_mask;         /* [B] or NULL: index of the mask that passed, -1: none                         */
    int32_t  *hit_rank;         /* [B] or NULL: rank r of the output path                                       */
    double   *metric;           /* [B] or NULL: the output path's metric                                        */
} qpd_search_args;
int qpd_decode_search(qpd_decoder *dec, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                      const qpd_search_args *sr, void *stream);
int qpd_decode_search_host(qpd_decoder *dec, const void *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                           const qpd_search_args *sr);

/*
 * Blind-detection metric (D-metric): the cheap half of PDCCH blind detection, one
 * double per candidate frame, by which a receiver ranks its candidates before it
 * runs the list decode above on the best few.  The counterpart of the reference's
 *     DMetricCalculator::calculate(llr) -> double
 *         PolarEncoder/PolarBD/_cpp/src/DMetric.cpp:24-177
 * batched: the float FastSC traversal (FastSCDecoder.cpp:21-151; the same f / g / u,
 * `<= 0` decisions and SPC rule) plus one accumulator per frame, which starts at 0
 * (:36) and, in traversal order, adds (sum of the node's LLRs) / size at every R0
 * node (:57-62) and |sum| / size at every REP node (:91-97), the sums sequential in
 * element order; R1, SPC and unlabelled nodes and the leaves add nothing.
 * metric[f] is that double, bit for bit.  (DMetric.cpp's depth -1 case, a labelled
 * root, cannot arise: qpd_create refuses such a node_type.)
 *
 * dec: a QPD_FASTSC_FLOAT decoder -- its frozen_bits and node_type are the
 * calculator's; QPD_E_INVALID for every other kind (qpd_last_error names it).
 * llr: float64 [B][N].  metric: float64 [B], required (QPD_E_INVALID if NULL).
 * out: uint8 [B][K], or NULL for the metric alone; when given it receives exactly
 * qpd_decode_f64's bits for the same input (the calculator itself returns none).
 * Device pointers in qpd_dmetric, host pointers in qpd_dmetric_host.  Frames >= B
 * are never written, in either output.  The refusals return before any launch.
 * Stream ordering, the per-handle lock and qpd_info.last_engine as for
 * qpd_decode_f64; the host variant keeps qpd_decode_f64_host's host_max_frames
 * dispatch (qpd_set_host_engine honoured).
 */
int qpd_dmetric(qpd_decoder *dec, const double *d_llr, int64_t B, double *d_metric, uint8_t *d_out, void *stream);
int qpd_dmetric_host(qpd_decoder *dec, const double *h_llr, int64_t B, double *h_metric, uint8_t *h_out);

/* Returns QPD_E_INPUT (and clears the flags) if any decode since the last
 * check saw a channel symbol outside [0, v), a Lloyd bisect index outside
 * the reconstruction list, or a NaN path metric reaching a list selection
 * (each undefined behaviour in the reference), or a NaN LLR in qpd_quantize_llr /
 * qpd_decode_llr, or a message byte other than 0 / 1 in qpd_encode / qpd_tx_frames;
 * waits for the decoder's previous work (not the whole device). */
int qpd_check_input_error(qpd_decoder *dec);

/*
 * GPU-resident Monte-Carlo frames (replaces the driver loop
 * mainQuantizedDecoder_LLRDomain.py:151-176): for global frame ids
 * [frame0, frame0+B): message bits, polar encoding (x = u F^{(x)n}, natural
 * order), BPSK, AWGN (std sigma), LLR = 2y/sigma^2 and the driver's channel
 * quantizer (<= edges[0] -> 0, >= edges[M] -> q-1, else
 * lut[bisect_left(edges[:M], llr) - 1]).  Random numbers are Philox4x32-10 of
 * (seed, global frame id), so frames do not depend on batching or sharding.
 * d_msg: device uint8 [B][K]; d_symbols: device int32 [B][N].  For the
 * CRC-aided kinds the message is A random bits followed by the first K-A bits
 * of their CRC (the driver's CRCEnc, mainQuantizedDecoder_LLRDomain.py:153-156),
 * and d_msg holds the A message bits ([B][A]).
 * Alignment of d_msg (all four qpd_mc_* entry points): where a row is a
 * multiple of 8 bytes (K % 8 == 0, or A % 8 == 0 for the CRC-aided kinds) the
 * generator stores it 8 bytes at a time and d_msg must be 8-byte aligned --
 * QPD_E_INVALID otherwise, before anything is launched; any other row length
 * takes any base.  d_out takes any base (the counters of d_counts fall back to
 * a byte loop).
 */
typedef struct qpd_mc_channel {
    double sigma;           /* AWGN standard deviation                 */
    int32_t q;              /* number of channel symbols               */
    int32_t n_edges;        /* M+1, 2..257                             */
    const double *edges;    /* host [n_edges], ascending               */
    const int32_t *lut;     /* host [n_edges-1], values in [0, q)      */
} qpd_mc_channel;
int qpd_mc_frames(qpd_decoder *dec, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B,
                  uint8_t *d_msg, int32_t *d_symbols, void *stream);
/* The same frames, decoded: d_out = what qpd_decode returns for the symbols
 * qpd_mc_frames generates with the same arguments (d_msg as there), without
 * materializing the int32 symbols -- on a fast-engine decoder in pre-mode the
 * generator writes the root pre-pass rows the decode kernel reads (LUT kinds;
 * q <= v).  d_counts (device int64[2], or NULL): bit errors and block errors of
 * the B frames (d_out against d_msg) are ADDED to it, the driver's counters
 * (:181-183).  The driver's loop body (mainQuantizedDecoder_LLRDomain.py:151-183)
 * in one call. */
int qpd_mc_decode(qpd_decoder *dec, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B,
                  uint8_t *d_msg, uint8_t *d_out, int64_t *d_counts, void *stream);
/*
 * The same frames for the float64-LLR decoders (the drivers mainFPDecoder.py and
 * mainQuantizedDecoder_ContinuousDomain.py): d_llr, device float64 [B][N], holds
 * the LLRs 2y/sigma^2 themselves -- the doubles qpd_mc_frames quantizes, so for
 * one (seed, frame id) a float decoder and a LUT decoder of the same code see the
 * same message and noise, and quantizing d_llr with the driver's rule gives
 * qpd_mc_frames' symbols bit for bit.  Any decoder kind (the code is what counts);
 * d_msg as for qpd_mc_frames.  d_llr needs 8-byte alignment; 16 is faster.
 * rec == NULL: only ch->sigma is read (edges / lut may be NULL, n_edges 0).
 * rec != NULL (host [q], finite, q <= 256): the continuous-domain driver's channel
 * quantizer -- d_llr holds rec[s], s the symbol qpd_mc_frames writes for that LLR
 * (saturations included; a uniform and a Lloyd design are both edges plus
 * reconstruction values).
 * A CRC-aided decoder whose K - A exceeds crc_n (QPD_CASCL_FLOAT with
 * A + crc_n < K) has no CRC bits to fill its message with: QPD_E_UNSUPPORTED.
 */
int qpd_mc_llr(qpd_decoder *dec, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0, int64_t B,
               uint8_t *d_msg, double *d_llr, void *stream);
/* qpd_mc_llr's frames, decoded: d_out = what qpd_decode_f64 returns for them
 * (float64-LLR kinds only: QPD_SC_FLOAT, 7..14; QPD_E_INVALID otherwise); d_msg,
 * d_counts, stream ordering and qpd_info.last_engine as for qpd_mc_decode.  The
 * LLRs pass through a buffer of the decoder's own, chunk by chunk:
 *     frames per chunk = max(1, 2^28 / (8 N))      (at most 256 MB of LLRs;
 * halved while the allocation fails, like the other chunk buffers), each chunk
 * generated, then decoded, then the counters over the whole range. */
int qpd_mc_decode_f64(qpd_decoder *dec, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0,
                      int64_t B, uint8_t *d_msg, uint8_t *d_out, int64_t *d_counts, void *stream);

/*
 * The transmit side for messages the caller chooses.  Replaces the package every
 * reference driver imports and the reference does not ship,
 *     PolarBDEnc.Encoder.PolarEnc   PolarEnc(N, K, frozenbits, msgbits).encode(msg)
 *     PolarBDEnc.Encoder.CRCEnc     CRCEnc(crc_n, crc_p).encode(msg)
 *         mainQuantizedDecoder_LLRDomain.py:10-11, :72-73, :153-158; mainFPDecoder.py:12-13
 * (the CRC is CRC::encoding, utils.cpp:77-92, over the handle's taps), batched, and
 * the drivers' channel behind it (mainQuantizedDecoder_LLRDomain.py:161-176) for such
 * messages: qpd_mc_frames / qpd_mc_llr with the message given instead of drawn.
 *
 * dec: any decoder kind -- its code (N, K, frozen_bits) and, for the CRC-aided
 * kinds, its A, crc_n and taps are what counts.  msg: uint8 [B][A] for the CRC-aided
 * kinds, [B][K] otherwise, entries 0 / 1.  The information bits are the message, for
 * the CRC-aided kinds followed by the first K - A bits of its check code; u[information
 * positions] = information bits, frozen positions 0, codeword x = u F^{(x)n} in natural
 * order, one byte per bit.
 * qpd_tx_args (may be NULL: no mask, signal present):
 *   crc_mask / crc_mask_bits  a mask for the check code (e.g. an RNTI), placed as in
 *       qpd_status_args: mask bit l is XORed onto check-code bit crc_n - crc_mask_bits
 *       + l, before the check code is cut to its first K - A bits -- the mirror of
 *       qpd_decode_status's compare, so a word encoded under a mask and decoded
 *       noiselessly under the same mask passes.  One mask per call.  QPD_E_INVALID on a
 *       kind without CRC, for crc_mask_bits outside [0, crc_n], a NULL mask with
 *       bits > 0, or an entry above 1.
 *   no_signal  qpd_tx_frames only (QPD_E_INVALID in qpd_encode*): 1 = y = sigma *
 *       noise, the BPSK term dropped and nothing else -- a candidate nothing was sent
 *       in.  The outputs then do not depend on d_msg, which may be NULL.
 * A CRC-aided code with K - A > crc_n (QPD_CASCL_FLOAT with A + crc_n < K) has no check
 * bits to fill its message with: QPD_E_UNSUPPORTED, as in qpd_mc_llr.
 * A message byte other than 0 / 1 is undefined in the reference; here it counts as its
 * low bit and raises the decoder's input-error word (qpd_check_input_error; the host
 * variant returns QPD_E_INPUT, its outputs written); the other frames are unaffected.
 *
 * qpd_encode: device pointers; d_info ([B][K]) and d_codeword ([B][N]) may each be
 * NULL, both NULL is QPD_E_INVALID.  qpd_encode_host: the same from host buffers,
 * always on the host (the same word-packed algorithm; no crossover to the device).
 *
 * qpd_tx_frames: the received frames of global frame ids [frame0, frame0 + B) for
 * d_msg ([B] rows), d_frames [B][N] by out_type: int32 symbols, uint8 symbols (the
 * int32 symbol narrowed; q <= 256, QPD_E_INVALID otherwise) or float64 LLRs.  The
 * noise of (seed, frame id, position) is qpd_mc_frames' noise -- the same Philox
 * counter and arithmetic, quantizer and rec rule: when d_msg holds the messages
 * qpd_mc_frames wrote for the range, d_frames is that call's symbols, or qpd_mc_llr's
 * doubles, bit for bit.  ch as for qpd_mc_frames (symbols) / qpd_mc_llr (LLRs); rec
 * applies to QPD_TX_LLR_F64 only (QPD_E_INVALID with the symbol outputs).
 *
 * Any base address for d_msg, d_info, d_codeword and uint8 d_frames: rows that are a
 * multiple of 8 bytes on an 8-byte aligned base are moved 8 bytes at a time (uint8
 * symbols: 2 on an even base), everything else byte by byte.  int32 / float64
 * d_frames need their type's alignment (QPD_E_INVALID otherwise; 8 / 16 bytes are the
 * fast cases).  Frames >= B and bytes past the last row are never written.  All
 * refusals return before any launch, qpd_last_error naming the argument.  Stream
 * ordering and the per-handle lock as for qpd_mc_frames.
 */
typedef struct qpd_tx_args {
    const uint8_t *crc_mask;   /* host, [crc_mask_bits] of 0/1, or NULL; placed as in qpd_status_args */
    int32_t crc_mask_bits;     /* 0..crc_n */
    int32_t no_signal;         /* qpd_tx_frames only: 1 = y = sigma * noise (no BPSK term): an empty candidate */
} qpd_tx_args;
int qpd_encode(qpd_decoder *dec, const uint8_t *d_msg, int64_t B, const qpd_tx_args *tx, uint8_t *d_info,
               uint8_t *d_codeword, void *stream);
int qpd_encode_host(qpd_decoder *dec, const uint8_t *h_msg, int64_t B, const qpd_tx_args *tx, uint8_t *h_info,
                    uint8_t *h_codeword);
enum qpd_tx_out { QPD_TX_SYM_I32 = 0, QPD_TX_SYM_U8 = 1, QPD_TX_LLR_F64 = 2 };
int qpd_tx_frames(qpd_decoder *dec, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0,
                  int64_t B, const uint8_t *d_msg, const qpd_tx_args *tx, int32_t out_type, void *d_frames, void *stream);

/*
 * LLRs on the LUT decoders: the driver's channel quantizer
 * (mainQuantizedDecoder_LLRDomain.py:167-176) on the device, in front of the
 * decode -- what qpd_decode_f64 is to the float64-LLR decoders.  ch: the
 * qpd_mc_channel above; sigma is not read (0 is fine); edges (ascending, n_edges
 * in 2..257) and lut (values in [0, q)) as for qpd_mc_frames.  Exactly that rule
 * for every double, +-inf and +-0 included:
 *     llr <= edges[0] -> 0,  llr >= edges[M] -> q-1,  else lut[bisect_left(edges[:M], llr) - 1];
 * a float32 LLR is widened to double first (exact).  A NaN has no symbol in the
 * driver: it is quantized to symbol 0 and raises the decoder's input-error word
 * (qpd_check_input_error / the host entry point: QPD_E_INPUT, as for a symbol
 * outside [0, v)); the other frames of the batch are not affected.
 * d_llr: device float64 or float32 [B][N] (llr_type), 8- / 4-byte aligned
 * (QPD_E_INVALID otherwise); 16-byte alignment is the fast case.  LUT kinds only
 * (QPD_E_INVALID for a float64-LLR decoder: use qpd_decode_f64).  Stream
 * ordering, the per-handle lock and qpd_info.last_engine as for qpd_decode;
 * qpd_info.u8_staged is 0 after these calls.
 */
enum qpd_llr_type { QPD_LLR_F64 = 0, QPD_LLR_F32 = 1 };
/* The channel quantizer alone: d_symbols, device uint8 [B][N] (q <= 256). */
int qpd_quantize_llr(qpd_decoder *dec, const qpd_mc_channel *ch, const void *d_llr, int32_t llr_type, int64_t B,
                     uint8_t *d_symbols, void *stream);
/* Quantize + decode: d_out = what qpd_decode_u8 returns for qpd_quantize_llr's
 * symbols (q <= v).  A fast-engine decoder in pre-mode never sees the symbols:
 * the quantizer writes the root pre-pass rows the decode kernel reads, chunk by
 * chunk (one front launch per chunk, timed as QPD_KC_PRE); every other decoder
 * gets int32 symbols in the staging buffer qpd_decode_u8 uses. */
int qpd_decode_llr(qpd_decoder *dec, const qpd_mc_channel *ch, const void *d_llr, int32_t llr_type, int64_t B,
                   uint8_t *d_out, void *stream);
/* The same from host buffers, synchronous: the LLRs are quantized on the host
 * (the same function), then as qpd_decode_u8_host -- the host engine up to
 * qpd_info.host_max_frames frames, the GPU above, qpd_set_host_engine honoured. */
int qpd_decode_llr_host(qpd_decoder *dec, const qpd_mc_channel *ch, const void *h_llr, int32_t llr_type, int64_t B,
                        uint8_t *h_out);

/*
 * Offline table design (host code, no device needed) -- the reference's
 * MinDistortion LUT generator without OpenCV.
 *
 * qpd_optls_quantizer  <- LLRQuantizer::find_OptLS_quantizer
 *                         Quantizers/quantizers/_cpp/LLRQuantizer/LLRQuantizer.cpp:67-165
 *                         (Python twin QuantizeDensityEvolution/MinDistortionQuantizer.py:28-99):
 *   merge M LLR quanta (any order; density-weighted) into K groups of
 *   consecutive sorted quanta with minimum squared error.  Outputs
 *   density[K], quanta[K] (density-weighted means), lut[M] (symbol -> group)
 *   and the minimum distortion.
 * qpd_lutgen_mindistortion <- LLRQuantizerSC.run
 *                         QuantizeDensityEvolution/QLLRDensityEvolution_MinDistortion.py:73-126:
 *   density evolution of the v-level channel (density/quanta [v]) down the
 *   code tree; per node p = 2^depth + node - 1 one f table lut_f[p][a][b] and
 *   one g table lut_g[p][u][a][b] (uint8, [N-1][v][v] / [N-1][2][v][v]), and
 *   the evolved llr_density / llr_quanta [log2(N)+1][N][v] (llr_quanta is
 *   the decoders' virtual_channel_llr).  threads <= 0: all host cores.
 * sum_order: QPD_SUM_SEQUENTIAL = the C++ quantizer the reference generator
 * calls; QPD_SUM_NUMPY = its numpy twin (pairwise sums).  Returns 0, -1 on bad
 * arguments, -2 if a node has fewer than v distinct values (the reference
 * aborts there: CV_Assert(M >= K)).
 */
enum qpd_sum_order { QPD_SUM_SEQUENTIAL = 0, QPD_SUM_NUMPY = 1 };
int qpd_optls_quantizer(const double *density, const double *quanta, int32_t M, int32_t K, int32_t sum_order,
                        double *out_density, double *out_quanta, int32_t *out_lut, double *out_distortion);
int qpd_lutgen_mindistortion(int32_t N, int32_t v, const double *ch_density, const double *ch_quanta,
                             int32_t sum_order, int32_t threads, uint8_t *lut_f, uint8_t *lut_g,
                             double *llr_density, double *llr_quanta);

/* Introspection for tests / benchmarks. */
typedef struct qpd_info {
    int32_t kind, N, K, L, v;
    int32_t num_ops;          /* length of the static traversal schedule     */
    int32_t frames_per_wave;  /* frames decoded by one 64-lane wavefront     */
    int32_t lanes_per_frame;  /* lane stride of one frame (pow2 >= L)        */
    int32_t max_waves;        /* persistent grid cap                         */
    int64_t scratch_bytes_per_wave;
    int32_t engine;           /* enum qpd_engine actually used               */
    int32_t lds_bytes_per_wave;
    int32_t lds_from_depth;   /* fast engine: tree depths >= this live in LDS */
    int32_t out_bits;         /* bits per decoded frame: K, or A (CRC-aided)  */
    int64_t host_max_frames;  /* host-buffer calls of up to this many frames run
                                 on the host engine (qpd_set_host_engine); 0: none */
    int32_t prefix_ops;       /* fast engine, list kinds: ops of the frozen prefix run
                                 once per frame by lut_prefix_kernel (0: no split);
                                 num_ops counts both parts */
    int32_t last_engine;      /* enum qpd_ran: what decoded the handle's last decode
                                 call (tests assert that a "GPU" case ran the kernels) */
    int64_t lookups_per_path; /* f/g table lookups one path of one frame makes in the
                                 reference's traversal of this code (N log2 N for the
                                 SC/SCL kinds; fewer where special nodes skip subtrees):
                                 the algorithmic unit of the roofline (bench.py) */
    int32_t fast_variant;     /* fast engine: which decode kernel instantiation the plan
                                 runs -- bit 0: one pointer word per path (PW1); bit 1:
                                 the general special-node instantiation (R1L: R1 nodes
                                 beyond the LDS tail or without op-record ranks, R0 / REP
                                 nodes without one quanta row); 0 otherwise */
    int32_t u8_staged;        /* 1: the handle's last decode call widened uint8 input into the
                                 int32 staging buffer (qpd_decode_u8 / _u8_host outside pre-mode);
                                 0: int32 and float64 calls, host-engine runs, uint8 read directly */
} qpd_info;
/* qpd_info.last_engine: no decode yet, the GPU kernels (qpd_decode*, the GPU
 * branch of the host-buffer calls, qpd_mc_decode, qpd_mc_decode_f64), or the
 * host engine. */
enum qpd_ran { QPD_RAN_NONE = 0, QPD_RAN_GPU = 1, QPD_RAN_HOST = 2 };
int qpd_get_info(const qpd_decoder *dec, qpd_info *info);

/*
 * Kernel timing for benchmarks (no reference counterpart).  While enabled,
 * every kernel launch of this handle is bracketed by HIP events recorded on
 * the launch stream; qpd_kernel_times waits for them and returns, per kernel
 * class, the summed durations (ms) and the number of launches since the last
 * call, then forgets them.  Arrays have QPD_KC_COUNT entries.
 */
enum qpd_kernel_class {
    QPD_KC_PRE = 0,    /* root_pre_kernel (fast engine, root pre-pass); llr_front_kernel (the LLR calls) */
    QPD_KC_DECODE = 1, /* lut_fast_kernel / generic_decode_kernel                   */
    QPD_KC_MC = 2,     /* mc_frames_kernel (qpd_mc_frames, qpd_mc_llr, both fused calls) */
    QPD_KC_PFX = 3,    /* lut_prefix_kernel (fast engine, frozen prefix of list kinds) */
    QPD_KC_COUNT = 4
};
int qpd_profile(qpd_decoder *dec, int32_t enable);
int qpd_kernel_times(qpd_decoder *dec, double *ms, int64_t *launches);

/*
 * On-chip peak probe (no reference counterpart): the LDS-path rate of one
 * instruction with every CU busy, measured on `device` by a streaming
 * microbenchmark (independent chains, 16 wave-instructions in flight per
 * wave, 8 waves per CU).  op: QPD_PROBE_BPERMUTE (ds_bpermute_b32, the
 * decoder's table lookups and fork copies), QPD_PROBE_READ_B32 (ds_read_b32,
 * its LDS rows), QPD_PROBE_READ_B64.  *gbps = bytes moved (64 lanes x width
 * per wave-instruction) / s.
 */
enum qpd_probe_op { QPD_PROBE_BPERMUTE = 0, QPD_PROBE_READ_B32 = 1, QPD_PROBE_READ_B64 = 2 };
int qpd_probe_lds(int32_t device, int32_t op, double *gbps);

#ifdef __cplusplus
}
#endif
#endif /* QPD_H */
