/*
 * afsk_amd.h -- C-ABI of libafsk_amd.so: the MI355X (gfx950) batched AFSK
 * demodulation path behind lavajuno/afskmodem's Receiver.
 *
 * The reference has no FFI: its hot path is the private method
 *     Receiver.__decodeBits(frames) -> str          (afskmodem.py:354-381)
 * followed by ECC.decode + __bitsToBytes           (afskmodem.py:154-163, 393-399)
 * called from Receiver.load (:420-430) and Receiver.receive (:402-417).
 * The entry points below are what a ctypes binding inside afskmodem.py would
 * bind to replace exactly that span (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types cross this boundary;
 *  - every function returns 0 on success or a negative AFSK_E_* code and never
 *    throws; afsk_last_error() returns the message of the calling thread's
 *    last failure;
 *  - the caller owns every buffer.  Unless a function name ends in _host, all
 *    data pointers are DEVICE pointers of the current HIP device and the call
 *    is asynchronous on `hip_stream` (a hipStream_t, NULL = default stream);
 *  - there is no CPU fallback: without a HIP device every compute entry fails
 *    with AFSK_E_NO_DEVICE;
 *  - host threads (the I/O pool of the file entries, the staging copies of the
 *    _host entries) are sized by the CPUs the process may really use: the
 *    cgroup CPU quota / affinity mask, divided by LOCAL_WORLD_SIZE when that is
 *    set (one process per GPU: the ranks of a node share the node's CPUs);
 *    AFSK_IO_THREADS / AFSK_COPY_THREADS override.
 */
#ifndef AFSK_AMD_H
#define AFSK_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFSK_ABI_VERSION 2 /* 2: afsk_group_plan_* / afsk_demod_batch_grouped, AFSK_ST_BAD_LENGTH, afsk_wav_egress;
                              the live entries and, after them, the per-channel-rate *_mixed entries are additions
                              to version 2 */

/* return codes */
#define AFSK_OK 0
#define AFSK_E_INVALID_ARG (-1)
#define AFSK_E_INVALID_BAUD (-2) /* bit_frames not a multiple of 4 or 2*bf >= 4096      */
#define AFSK_E_NO_DEVICE (-3)
#define AFSK_E_HIP (-4)          /* a HIP runtime call failed, see afsk_last_error      */
#define AFSK_E_HOST (-5)         /* host-side failure in a host-buffer entry (out of memory,
                                    thread creation); nothing is thrown across the boundary */

/* per-stream status written to out_status (reference behaviour in brackets) */
#define AFSK_ST_OK 0
#define AFSK_ST_TOO_SHORT 1 /* len < 4096 [__recoverClockIndex -> -1 -> "" , :323-325] */
#define AFSK_ST_NO_DATA 2   /* no terminator / zero bits [bits == "" -> b"", :422-424]  */
#define AFSK_ST_INVALID_BAUD 3 /* bit_frames[s] rejected (host wrappers raise before launch) */
#define AFSK_ST_BAD_LENGTH 4 /* stream_len[s] < 0 or > AFSK_MAX_STREAM_LEN: refused by the kernel before any
                                sample is addressed (the device entries never see the length array on the
                                host; the host entries reject such a batch with AFSK_E_INVALID_ARG) */

/* Fixed constants of the reference that the kernels compile in. */
#define AFSK_SAMPLE_RATE 48000 /* :69,71,187,233,260,277 */
#define AFSK_SYNC_WINDOW 4096  /* :323,327                */
#define AFSK_DEAD_ZONE 512     /* :290-292                */
#define AFSK_TAIL_SILENCE 4800 /* :468                    */
/* Longest stream the kernels address with 32-bit byte offsets (about 6.2 hours of audio). */
#define AFSK_MAX_STREAM_LEN ((1 << 30) - (1 << 15))

int afsk_version(void);
/* Copies the calling thread's last error message (NUL terminated, truncated to
 * cap) and returns its full length. */
int afsk_last_error(char *buf, int cap);
/* Number of visible HIP devices (0 when there is none); never fails. */
int afsk_device_count(void);
/* hipStreamSynchronize(hip_stream). */
int afsk_sync(void *hip_stream);

/*
 * Replaces Receiver.__decodeBits (:354-381) + ECC.decode (:154-163) +
 * __bitsToBytes (:393-399) for n_streams independent streams at once.
 *
 *  samples        int16 mono 48 kHz, all streams in one allocation
 *  stream_offset  [n] first sample of stream s, in samples from `samples`.  Any value works (streams
 *                 need 2-byte alignment only); EVEN offsets from a dword-aligned `samples` -- best:
 *                 multiples of 8 samples -- run at full speed: a stream that starts on an odd sample
 *                 is fetched by 2-byte-aligned requests, about 25 % slower (same results)
 *  stream_len     [n] length of stream s in samples (0 ... AFSK_MAX_STREAM_LEN; anything else:
 *                 status AFSK_ST_BAD_LENGTH for that stream, its neighbours are unaffected)
 *  bit_frames     [n] 48000 / baud of stream s (Receiver.__init__ :277);
 *                 must be a multiple of 4 with 2*bit_frames < 4096
 *  amp_end_threshold  Receiver(amp_end_threshold=...) (:276), squelch of :375
 *  out_bytes      [n, out_stride] decoded payload bytes (row s, first
 *                 min(out_nbytes[s], out_stride) bytes are written; any
 *                 stride works -- rows of more than ~200 bytes are cheapest
 *                 when out_bytes and out_stride are multiples of 128: what a
 *                 launch pays for its output is the number of cache lines
 *                 it dirties)
 *  out_nbytes     [n] number of decoded bytes (may exceed out_stride: the row
 *                 was then truncated; size rows as stream_len/(14*bf)+1)
 *  out_nbits      [n] coded bits demodulated incl. ECC (debug line :380)
 *  out_clock_idx  [n] recovered clock index (:338), -1 when too short
 *  out_term_frame [n] frame index after the training terminator (:368), -1
 *                 when too short
 *  out_status     [n] AFSK_ST_*
 *
 * Results are bit-exact with the reference for every input (integer path).
 */
int afsk_demod_batch(const int16_t *samples, const int64_t *stream_offset,
                     const int32_t *stream_len, const int32_t *bit_frames,
                     int32_t amp_end_threshold, int32_t n_streams, uint8_t *out_bytes,
                     int32_t out_stride, int32_t *out_nbytes, int32_t *out_nbits,
                     int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                     void *hip_stream);

/*
 * afsk_demod_batch plus two optional soft outputs (either may be NULL), for callers that
 * want link-quality figures without a second pass over the samples.  Both are values the
 * reference computes and discards:
 *
 *  out_corrected  [n] codewords of ECC.decode's input (floor(nbits/7) of them, :156-157) whose
 *                 syndrome (:146-147) was non-zero, i.e. single-bit corrections applied.  0 for a
 *                 stream the demodulator refuses (status AFSK_ST_TOO_SHORT, AFSK_ST_INVALID_BAUD or
 *                 AFSK_ST_BAD_LENGTH), whatever the array held before the call -- in every entry
 *                 that takes out_corrected
 *  out_margins    [n, margin_stride] per demodulated symbol k (sample clock_idx + k*bf),
 *                 space_diff - mark_diff of __decodeBit (:348-349): > 0 decodes as 1, <= 0
 *                 as 0 (:350-351).  Written for the symbols the reference demodulated:
 *                 k < (term_frame - clock_idx)/bf + nbits when a terminator was found, else
 *                 every k with clock_idx + k*bf < len - bf; entries past that (and past
 *                 margin_stride) are unspecified/not written.
 */
int afsk_demod_batch_ex(const int16_t *samples, const int64_t *stream_offset,
                        const int32_t *stream_len, const int32_t *bit_frames,
                        int32_t amp_end_threshold, int32_t n_streams, uint8_t *out_bytes,
                        int32_t out_stride, int32_t *out_nbytes, int32_t *out_nbits,
                        int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                        int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride,
                        void *hip_stream);

/*
 * The Receiver-shaped form of afsk_demod_batch_ex: ONE bit_frames for every stream of the
 * launch, passed by value.  A Receiver has exactly one baud rate (Receiver.__init__ :275-284:
 * bit_frames, the two tone templates and the training cycle are per-object constants), so a batch
 * decoded on behalf of one Receiver never needs the per-stream array.  bit_frames is validated on
 * the host (AFSK_E_INVALID_BAUD) and selects a kernel compiled for exactly that geometry -- no
 * per-stream load of it, no geometry switch in the kernel.  Same outputs, bit for bit, as
 * afsk_demod_batch_ex with bit_frames[s] == bit_frames for all s; out_corrected / out_margins may
 * be NULL (margin_stride 0).
 */
int afsk_demod_batch_uniform(const int16_t *samples, const int64_t *stream_offset,
                             const int32_t *stream_len, int32_t bit_frames,
                             int32_t amp_end_threshold, int32_t n_streams, uint8_t *out_bytes,
                             int32_t out_stride, int32_t *out_nbytes, int32_t *out_nbits,
                             int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                             int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride,
                             void *hip_stream);

/*
 * Rate-grouped dispatch of a MIXED-baud batch whose bit_frames the HOST can see (a list of Receivers of
 * different baud rates, each with its own streams: one baud rate per Receiver, :275-284; streams are
 * independent, :354-381).  The plan buckets the streams by bit_frames once (a stable sort on the host, one
 * upload of an index list + the bit_frames, 8 bytes per stream); afsk_demod_batch_grouped then decodes the
 * batch with ONE kernel launch that walks the streams bucket by bucket (inside windows of 4096 consecutive streams,
 * 8192 for a ragged plan, so that the streams in flight stay close in memory), so that the wavefronts resident on a
 * compute unit run the same rate's code: 3 - 12 % faster than stream order when four or more rates are mixed
 * (below that the plan keeps stream order; one rate: the kernel of afsk_demod_batch_uniform).  Nothing but a
 * kernel launch (with out_corrected: a small kernel that zeroes it first): asynchronous on hip_stream like every device entry, safe inside a stream capture, and
 * calls may share a plan freely.  Outputs land at the ORIGINAL stream numbers, bit for bit what
 * afsk_demod_batch_ex writes for the same bit_frames[] (a stream with an invalid bit_frames gets status
 * AFSK_ST_INVALID_BAUD).  afsk_demod_batch (bit_frames[] in device memory, streams in the caller's order)
 * stays the entry for rates only the device knows.
 * (One launch of the uniform kernel per rate on forked HIP streams was measured and rejected: DESIGN.md 4.4.)
 *
 *  afsk_group_plan_create   bit_frames_host: HOST array [n].  Allocates 8 n bytes on the current device and
 *                           fills them (synchronous).
 *  afsk_group_plan_create_ragged  (r6, an addition: ABI version unchanged) the same with stream_len_host, a HOST
 *                           array [n] of the lengths the launches will be given (NULL = afsk_group_plan_create).  One
 *                           wavefront decodes one stream whatever its length and a workgroup of four keeps its share of
 *                           a CU until its longest stream ends, so when the lengths differ (shortest below 3/4 of the
 *                           longest) the walk takes, inside every window of 8192 consecutive streams (twice the
 *                           window of a rate-only plan; AFSK_GROUP_WINDOW, when set, is both) and every rate, the
 *                           LONGEST streams first -- also for a one-rate batch, whose uniform kernel then walks the
 *                           list.  Results do not depend on it (same outputs at the same stream numbers); lengths that
 *                           differ from those given later only cost speed.  The host entries do this by themselves.
 *  afsk_group_plan_info     n_streams, number of buckets, and per bucket (first `cap` of them, in launch
 *                           order: largest first) its bit_frames (0 = the refused streams) and stream count;
 *                           any pointer may be NULL
 *  afsk_demod_batch_grouped every array as afsk_demod_batch_ex, indexed by the original stream number;
 *                           n_streams is the plan's
 *  afsk_group_plan_destroy  after the launches that use the plan have completed (NULL is fine)
 */
typedef struct afsk_group_plan afsk_group_plan;
int afsk_group_plan_create(const int32_t *bit_frames_host, int32_t n_streams, afsk_group_plan **out_plan);
int afsk_group_plan_create_ragged(const int32_t *bit_frames_host, const int32_t *stream_len_host, int32_t n_streams,
                                  afsk_group_plan **out_plan);
int afsk_group_plan_info(const afsk_group_plan *plan, int32_t *out_n_streams, int32_t *out_n_groups,
                         int32_t *out_group_bit_frames, int32_t *out_group_count, int32_t cap);
int afsk_group_plan_destroy(afsk_group_plan *plan);
int afsk_demod_batch_grouped(const afsk_group_plan *plan, const int16_t *samples,
                             const int64_t *stream_offset, const int32_t *stream_len,
                             int32_t amp_end_threshold, uint8_t *out_bytes, int32_t out_stride,
                             int32_t *out_nbytes, int32_t *out_nbits, int32_t *out_clock_idx,
                             int32_t *out_term_frame, int32_t *out_status, int32_t *out_corrected,
                             int32_t *out_margins, int32_t margin_stride, void *hip_stream);

/*
 * Sequence-parallel demodulation (an addition: ABI version unchanged) for batches of FEW, LONG streams -- one long
 * recording, a large payload, the live gate's bursts -- where one wavefront per stream cannot fill the device.  The
 * work of one stream is split over many wavefronts: clock recovery per stream, then per-symbol decisions and squelch
 * flags by SEGMENTS of segment_symbols symbols (any number of wavefronts per stream), then terminator scan, squelch
 * stop, Hamming decode and byte pack per stream -- three kernel launches in order on hip_stream (a captured graph of
 * them is a linear chain).  Outputs are bit for bit what afsk_demod_batch_ex writes for the same input, including
 * clock_idx / term_frame / nbits of NO_DATA, TOO_SHORT and BAD_LENGTH streams; row bytes past nbytes are untouched.
 * Only 1200 baud (bit_frames 40) has a tuned segment kernel; every other valid bit_frames is decoded correctly.
 *
 *  afsk_split_plan_create   stream_len_host / bit_frames_host: HOST arrays [n] (several rates may be mixed; invalid
 *                           bit_frames: AFSK_E_INVALID_BAUD; a length outside 0 ... AFSK_MAX_STREAM_LEN:
 *                           AFSK_E_INVALID_ARG).  segment_symbols: a multiple of 64, 0 = the default (1024).
 *                           The plan (segment table, per-stream scratch offsets) lives on the current device;
 *                           it is sized with ceil(len / bit_frames) symbols per stream (synchronous upload).
 *  afsk_split_plan_info     n_streams, number of segments, scratch bytes a launch needs; any pointer may be NULL
 *  afsk_split_scratch_bytes host-only (no device needed): what afsk_split_plan_create would report for these arguments
 *  afsk_demod_batch_split   every array as afsk_demod_batch_ex (n_streams is the plan's); d_scratch: caller-owned
 *                           device memory of the plan's scratch bytes, contents need not be initialised, one launch
 *                           at a time per scratch buffer.  A device stream_len[s] above the length the plan was built
 *                           for gives that stream AFSK_ST_BAD_LENGTH (so does the usual range rule); shorter lengths
 *                           are fine.  bit_frames come from the plan.
 *  afsk_split_plan_destroy  after the launches that use the plan have completed (NULL is fine)
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, SPLIT_SIGNATURES, apart from
 * the SIGNATURES table that mirrors the `int afsk_*(` declarations above one to one.)
 */
typedef struct afsk_split_plan afsk_split_plan;
extern int afsk_split_plan_create(const int32_t *stream_len_host, const int32_t *bit_frames_host, int32_t n_streams,
                           int32_t segment_symbols, afsk_split_plan **out_plan);
extern int afsk_split_plan_info(const afsk_split_plan *plan, int32_t *out_n_streams, int32_t *out_n_segments,
                         int64_t *out_scratch_bytes);
extern int afsk_split_plan_destroy(afsk_split_plan *plan);
extern int afsk_split_scratch_bytes(const int32_t *stream_len_host, const int32_t *bit_frames_host, int32_t n_streams,
                             int32_t segment_symbols, int64_t *out_scratch_bytes, int32_t *out_n_segments);
extern int afsk_demod_batch_split(const afsk_split_plan *plan, const int16_t *samples, const int64_t *stream_offset,
                           const int32_t *stream_len, int32_t amp_end_threshold, void *d_scratch,
                           uint8_t *out_bytes, int32_t out_stride, int32_t *out_nbytes, int32_t *out_nbits,
                           int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                           int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride, void *hip_stream);

/*
 * Same operation on HOST buffers: allocates device scratch, copies in, runs the
 * HIP kernel, copies out, synchronises.  This is the PCIe-inclusive convenience
 * path a single Receiver.load() uses; it is not the benchmarked entry.
 * Both host entries work on a private NON-BLOCKING HIP stream of the calling thread (never the
 * NULL stream): they do not synchronise with the caller's own streams or with calls made by
 * other threads, and may be called concurrently (the reference's Receivers are independent
 * objects, afskmodem.py:275-284).  The host can see bit_frames[] here: one value -> the uniform kernel of
 * afsk_demod_batch_uniform, several -> the rate-sorted launch of afsk_demod_batch_grouped.  stream_len[s] above AFSK_MAX_STREAM_LEN is rejected here (AFSK_E_INVALID_ARG).
 */
int afsk_demod_batch_host(const int16_t *samples, int64_t total_samples,
                          const int64_t *stream_offset, const int32_t *stream_len,
                          const int32_t *bit_frames, int32_t amp_end_threshold,
                          int32_t n_streams, uint8_t *out_bytes, int32_t out_stride,
                          int32_t *out_nbytes, int32_t *out_nbits, int32_t *out_clock_idx,
                          int32_t *out_term_frame, int32_t *out_status);

/*
 * Gather form of the host entry: stream s is the host array streams[s] of stream_len[s]
 * samples (no concatenated buffer needed -- e.g. one array per .wav file or per
 * Receiver.load()-style frame list).  The streams are packed through two pinned 32 MiB
 * windows by a few copy threads while the previous window is on the PCIe link, then
 * demodulated with one launch.  Calls serialise on the cached staging buffers.
 */
int afsk_demod_streams_host(const int16_t *const *streams, const int32_t *stream_len,
                            const int32_t *bit_frames, int32_t amp_end_threshold,
                            int32_t n_streams, uint8_t *out_bytes, int32_t out_stride,
                            int32_t *out_nbytes, int32_t *out_nbits, int32_t *out_clock_idx,
                            int32_t *out_term_frame, int32_t *out_status);

/* The host entries keep their device scratch (samples + results) allocated between
 * calls (and the gather entry its pinned windows), because hipMalloc of a large buffer costs
 * far more than the transfer; this frees them.
 * Safe to call at any time; the next host-entry call allocates again. */
int afsk_host_scratch_release(void);

/*
 * .wav container ingest at scale (replaces SoundInput.loadFromFile,
 * afskmodem.py:213-217, for many files).  Two steps so that the caller owns the device buffer:
 *
 * afsk_wav_probe   walks the RIFF chunks of every file exactly like the stdlib `wave` reader the
 *   reference calls (:214): 'RIFF' <size> 'WAVE', then chunks with even padding; 'fmt ' must
 *   come before 'data'; the walk stops at 'data'.  Like the reference, rate / width / channel
 *   count are NOT interpreted -- they only bound the byte count:
 *   readframes(getnframes()) returns (data_size / (channels * bytes_per_sample)) whole frames,
 *   clipped to what the file really holds.  Host-only (no HIP call); parallel over files.
 *     out_data_offset [n] byte offset of the data chunk's payload in the file
 *     out_data_bytes  [n] bytes readframes(getnframes()) would return (may be odd:
 *                         __convertFrames (:201-205) then drops the last byte)
 *     out_status      [n] AFSK_WAV_*; anything but AFSK_WAV_OK means "not a plain PCM RIFF file,
 *                         or unreadable" -- the Python host re-opens such a file with the stdlib
 *                         reader so that the caller sees the reference's own exception
 *
 * afsk_wav_upload  reads data_bytes[s] & ~1 bytes at data_offset[s] of file s with pread()
 *   STRAIGHT INTO the library's two pinned staging windows (one copy: page cache -> pinned
 *   memory, a few threads in parallel) and sends each window to
 *   d_samples[stream_offset[s] ..] while the next one is being filled.  stream_offset is in
 *   samples, ascending, streams must not overlap and must fit capacity_samples.  Synchronous for
 *   the caller, on the calling thread's private non-blocking stream (NOT ordered against the
 *   caller's own streams: work of the caller that still reads or writes the destination range
 *   must have completed before the call).  Device bytes written: the streams themselves, plus
 *   gaps of at most 256 bytes BETWEEN two consecutive streams (alignment padding), which are set
 *   to zero; a larger gap between two streams and everything outside the streams is not touched,
 *   so one buffer can be filled by several calls.  afsk_wav_probe is host-only and, like
 *   afsk_wav_upload's file reading, fork-safe (a forked child builds its own I/O thread pool).
 */
#define AFSK_WAV_OK 0
#define AFSK_WAV_IO 1          /* cannot open / read                                      */
#define AFSK_WAV_NOT_RIFF 2    /* no 'RIFF' .. 'WAVE' header                              */
#define AFSK_WAV_NO_DATA 3     /* 'fmt ' and/or 'data' chunk missing, or 'data' first     */
#define AFSK_WAV_FORMAT 4      /* format tag other than PCM, zero channels / sample width */
#define AFSK_WAV_SLOT 5        /* afsk_wav_ingest only: the data does not fit the caller's slot    */
int afsk_wav_probe(const char *const *paths, int32_t n_files, int64_t *out_data_offset,
                   int64_t *out_data_bytes, int32_t *out_status);
int afsk_wav_upload(const char *const *paths, const int64_t *data_offset, const int64_t *data_bytes,
                    const int64_t *stream_offset, int32_t n_files, int16_t *d_samples,
                    int64_t capacity_samples);

/*
 * The same ingest in ONE pass per file (what batch.load_wav_batch uses since r3):
 *
 * afsk_file_sizes  st_size of every file (-1: cannot stat), host-only, parallel.  A file's data chunk
 *   cannot be longer than the file, so the sizes give a device layout BEFORE any file is opened:
 *   slot i = the device range reserved for file i (slot_offset[i], slot_samples[i], in samples).
 * afsk_wav_ingest  per file: open, the chunk walk of afsk_wav_probe, pread of the data chunk straight
 *   into pinned memory, close -- pipelined against the H2D copies (four 16 MiB staging buffers; pool
 *   threads fill, the calling thread sends).  out_data_offset / out_data_bytes / out_status as
 *   afsk_wav_probe; the stream of file i is d_samples[slot_offset[i] .. + out_data_bytes[i] / 2).
 *   Device bytes written: every slot in full (the data, then zeros) and gaps of at most 256 bytes
 *   between consecutive slots (zeros); a file whose status is not AFSK_WAV_OK -- or whose data would not
 *   fit its slot: AFSK_WAV_SLOT -- leaves a zeroed slot for the caller to fill (batch.load_wav_batch
 *   re-opens it with the stdlib reader, so the caller sees the reference's own exception or data).
 *   Slots ascending, non-overlapping, inside capacity_samples.  Synchronous for the caller, on the
 *   calling thread's private non-blocking stream (same ordering contract as afsk_wav_upload); fork-safe.
 */
int afsk_file_sizes(const char *const *paths, int32_t n_files, int64_t *out_size_bytes);
int afsk_wav_ingest(const char *const *paths, int32_t n_files, const int64_t *slot_offset,
                    const int64_t *slot_samples, int16_t *d_samples, int64_t capacity_samples,
                    int64_t *out_data_offset, int64_t *out_data_bytes, int32_t *out_status);

/*
 * .wav EGRESS at scale (r4; the mirror image of afsk_wav_ingest, for Transmitter.save, afskmodem.py:481-484, of many
 * payloads): stream s of the device buffer, d_samples[stream_offset[s] .. + stream_len[s]), is written to paths[s] as the
 * file SoundOutput.writeToFile (:256-263) produces through the stdlib writer -- the canonical 44-byte RIFF/WAVE header
 * (PCM, 1 channel, 48000 Hz, 16 bit, data size 2 * stream_len[s]) followed by the samples.  (The decimate / duplicate
 * quirk of SoundOutput.__convertFrames, :239-244, is the MODULATOR's job: afsk_modulate_batch(wav_quirk = 1).)
 * stream_offset (samples, ascending, non-overlapping) and stream_len are HOST arrays.  The calling thread copies windows
 * of the device range into the pinned staging ring (D2H, two alternating streams) and pool threads write each window's
 * file pieces as soon as its copy has completed: one open / pwritev (header + data) / close per file that lies inside
 * one window.  Existing files are replaced.  out_status[s]: AFSK_WAV_OK or AFSK_WAV_IO (cannot create / write: that
 * file's problem, the batch goes on).  Synchronous for the caller, on the calling thread's private streams (work of the
 * caller that still writes the source range must have completed before the call); fork-safe like the ingest.
 */
int afsk_wav_egress(const char *const *paths, int32_t n_files, const int16_t *d_samples,
                    const int64_t *stream_offset, const int32_t *stream_len, int32_t *out_status);

/*
 * On-device input synthesis: Transmitter.__getFrames (:452-469) with ECC.encode
 * (:166-175) and, when wav_quirk != 0, SoundOutput.__convertFrames' decimate-by-2
 * + duplicate (:239-244), written to samples[stream_offset[s] .. +stream_len[s])
 * (truncated, or zero padded after the 4800-sample tail).
 *
 *  payload      uint8 [n, payload_stride]; payload_len [n] bytes used per row
 *  bit_frames   [n] 48000 / baud; a positive multiple of 4 (every baud rate the reference's
 *               Waveforms accept, :69-70/:81-82, gives one); any other value yields an
 *               all-zero stream (device arrays are not validated on the host).  Every multiple
 *               of 4 from 4 up to 2^20 = 1048576 is rendered, whether or not it divides 48000;
 *               a value above 2^20 yields the all-zero stream too
 *  ts_cycles    [n] int(baud * training_time / 2)   (:438)
 *  max_stream_len  host-side upper bound of stream_len[] (sizes the grid); a stream whose device-side
 *               stream_len[s] is negative or above it is skipped (nothing written for it)
 */
int afsk_modulate_batch(const uint8_t *payload, int32_t payload_stride,
                        const int32_t *payload_len, const int32_t *bit_frames,
                        const int32_t *ts_cycles, const int64_t *stream_offset,
                        const int32_t *stream_len, int32_t max_stream_len, int32_t n_streams,
                        int32_t wav_quirk, int16_t *samples, void *hip_stream);

/*
 * Batched replay of Receiver.__listen (:299-319) over finite captures: the live-input gate
 * that decides which 2048-frame blocks (:189, :209) of a continuous recording are handed to
 * __decodeBits.  Per capture, repeated receive() calls are emulated: each call discards one
 * block (:303), waits for a block with getAmplitude > amp_start_threshold (:306) and records
 * blocks up to and including the first one with getAmplitude < amp_end_threshold (:316).
 * Only whole blocks of the capture are considered (no timeout: the call scans to the end).
 *
 *  max_stream_len   host-side upper bound of stream_len[]; max_blocks = max_stream_len / 2048.  A capture
 *                   whose device-side stream_len[s] is negative or above it is refused:
 *                   out_n_bursts[s] = -1, no sample of it is read
 *  block_amp        workspace AND output, int32 [n, max_blocks]: int(sum|x| / 2048) per block
 *  out_n_bursts     [n] bursts found (<= max_bursts)
 *  out_burst_start  [n, max_bursts] first sample of burst k, relative to the stream start
 *  out_burst_len    [n, max_bursts] samples in burst k (a multiple of 2048)
 *  out_open_end     [n] 1 when the last burst reached the end of the capture without a quiet
 *                   block (a live receiver would still be recording)
 * The bursts are demodulated by passing stream_offset[s] + out_burst_start[s,k] and
 * out_burst_len[s,k] to afsk_demod_batch.
 *
 * afsk_gate_batch_slots (r6, an addition) does that arithmetic on the device as well: it also writes the bursts as
 * FIXED demodulator slots -- slot s * max_bursts + k = burst k of capture s:
 *  out_slot_offset  int64 [n, max_bursts] stream_offset[s] + out_burst_start[s,k]; 0 where capture s has fewer bursts
 *  out_slot_len     int32 [n, max_bursts] out_burst_len[s,k]; 0 where capture s has fewer bursts (afsk_demod_batch*
 *                   answers such a slot with AFSK_ST_TOO_SHORT and reads nothing)
 * so that  afsk_gate_batch_slots(...) ; afsk_demod_batch_uniform(samples, out_slot_offset, out_slot_len, bit_frames,
 * amp_end, n * max_bursts, ...)  on one stream is what repeated Receiver.receive() calls do (:402-417) for n captures,
 * with no host round trip in between (two launches + one: capturable into one HIP graph).
 */
int afsk_gate_batch(const int16_t *samples, const int64_t *stream_offset,
                    const int32_t *stream_len, int32_t max_stream_len,
                    int32_t amp_start_threshold, int32_t amp_end_threshold, int32_t n_streams,
                    int32_t max_bursts, int32_t *block_amp, int32_t *out_n_bursts,
                    int32_t *out_burst_start, int32_t *out_burst_len, int32_t *out_open_end,
                    void *hip_stream);
int afsk_gate_batch_slots(const int16_t *samples, const int64_t *stream_offset,
                          const int32_t *stream_len, int32_t max_stream_len,
                          int32_t amp_start_threshold, int32_t amp_end_threshold, int32_t n_streams,
                          int32_t max_bursts, int32_t *block_amp, int32_t *out_n_bursts,
                          int32_t *out_burst_start, int32_t *out_burst_len, int32_t *out_open_end,
                          int64_t *out_slot_offset, int32_t *out_slot_len, void *hip_stream);

/*
 * The live receiver (an addition: ABI version unchanged): Receiver.receive (:299-319, :402-417) for n_channels
 * independent channels whose audio arrives chunk by chunk -- an SDR channelizer, a network fan-in, many sound cards.
 * Nothing here opens an audio device: the chunks come from any int16 source.  A channel's STREAM is every chunk pushed
 * to it since creation or since the last flush / reset; the gate is gate_scan_kernel's state machine over the
 * stream's whole 2048-sample blocks (block k = samples [2048 k, 2048 k + 2048)): discard one block, wait for
 * amp > amp_start, record through the first block with amp < amp_end (inclusive), repeat; no timeout, and a block
 * may straddle two pushes.  Every burst that closes during a push is demodulated IN that push, as
 * afsk_demod_batch_uniform over exactly its recorded samples.  All state (the partial block, the stream position, the
 * gate) lives on the device: a push never synchronises with the host, so one push of a fixed chunk_len can be
 * captured into a HIP graph once and replayed for every chunk.
 *
 * Capacities (samples): max_burst_len (>= 4096) bounds the bursts that are stored and demodulated; max_chunk_len
 * bounds chunk_len.  With K = (2047 + max_chunk_len) / 2048 (the most whole blocks one push walks: a carry of 2047
 * samples plus the chunk) a push reports at most  slots = 1 + K / 3  bursts per channel: one burst already open can
 * close in the first block, every further one needs a discard, a start and an end block, and a flush adds the burst
 * still recording.  The bound is exact: for every K some push or flush fills every slot.
 *
 *  afsk_live_layout   host-only (no device needed): the slots per channel and the device state bytes
 *                     afsk_live_create would allocate for these arguments
 *  afsk_live_create   bit_frames as afsk_demod_batch_uniform (AFSK_E_INVALID_BAUD); amp_start / amp_end as
 *                     afsk_gate_batch; n_channels >= 1, 4096 <= max_burst_len <= AFSK_MAX_STREAM_LEN,
 *                     1 <= max_chunk_len <= AFSK_MAX_STREAM_LEN, n_channels * slots < 2^31.  Allocates the state
 *                     on the current device and zeroes it (synchronous); every channel starts a new stream.
 *  afsk_live_info     n_channels, slots, state bytes; any pointer may be NULL
 *  afsk_live_push     appends chunk_len samples (0 ... max_chunk_len) to EVERY channel: row c of the chunk starts at
 *                     chunk + c * chunk_row_stride (samples, 2-byte alignment: a column window of a [channels, time]
 *                     buffer is pushed without a copy; chunk may be NULL when chunk_len is 0).  flush != 0 then ends
 *                     every stream: a burst still recording is reported (whole blocks only, AFSK_LIVE_OPEN_END, as
 *                     afsk_gate_batch's open_end burst), the partial block is dropped, and the next push starts a new
 *                     stream at sample 0 with its discard block.  Outputs, slot c * slots + k = the k-th burst
 *                     channel c reported in this push:
 *                       out_n_closed    int32 [n_channels] slots of channel c in use
 *                       out_burst_start int64 [n_channels, slots] first sample of the burst in the channel's stream
 *                       out_burst_len   int32 [n_channels, slots] samples recorded (a multiple of 2048)
 *                       out_flags       int32 [n_channels, slots] AFSK_LIVE_* bits
 *                       out_bytes ... margin_stride  the DemodOutputs of afsk_demod_batch_uniform over the
 *                                       n_channels * slots slots (rows / arrays indexed by slot)
 *                     An unused slot has length 0 (flags 0), demod status AFSK_ST_TOO_SHORT and, like every
 *                     stream the demodulator refuses, 0 in out_corrected whatever the push before left there.  A burst longer than
 *                     max_burst_len is gated exactly like any other; the samples beyond the capacity are not stored,
 *                     and when it closes it is reported with its true start and length (at most 2^31 - 2048),
 *                     AFSK_LIVE_OVERFLOW and status AFSK_ST_TOO_SHORT: not demodulated.  chunk_len > max_chunk_len, a
 *                     receiver of another device or a NULL pointer: AFSK_E_INVALID_ARG.  Two launches in order on
 *                     hip_stream; pushes to one receiver must run in order (one stream, or ordered streams).
 *  afsk_live_reset    drops the state of every channel (d_mask_or_null NULL) or of the channels whose DEVICE uint8
 *                     mask entry is non-zero, without reporting anything: they start a new stream
 *  afsk_live_destroy  after the launches that use the receiver have completed (NULL is fine)
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_SIGNATURES.)
 */
#define AFSK_LIVE_OPEN_END 1 /* reported by a flush while still recording (no quiet block yet)           */
#define AFSK_LIVE_OVERFLOW 2 /* longer than max_burst_len: not stored in full, not demodulated             */
typedef struct afsk_live afsk_live;
extern int afsk_live_layout(int32_t n_channels, int32_t max_burst_len, int32_t max_chunk_len, int32_t *out_slots,
                            int64_t *out_state_bytes);
extern int afsk_live_create(int32_t n_channels, int32_t bit_frames, int32_t amp_start_threshold,
                            int32_t amp_end_threshold, int32_t max_burst_len, int32_t max_chunk_len, afsk_live **out);
extern int afsk_live_info(const afsk_live *live, int32_t *out_n_channels, int32_t *out_slots,
                          int64_t *out_state_bytes);
extern int afsk_live_push(afsk_live *live, const int16_t *chunk, int64_t chunk_row_stride, int32_t chunk_len,
                          int32_t flush, int32_t *out_n_closed, int64_t *out_burst_start, int32_t *out_burst_len,
                          int32_t *out_flags, uint8_t *out_bytes, int32_t out_stride, int32_t *out_nbytes,
                          int32_t *out_nbits, int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                          int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride, void *hip_stream);
extern int afsk_live_reset(afsk_live *live, const uint8_t *d_mask_or_null, void *hip_stream);
extern int afsk_live_destroy(afsk_live *live);

/*
 * Per-channel rates (added after ABI version 2; the version is unchanged): a live receiver or transmitter whose
 * channels each have their own bit_frames (and, for the transmitter, training length), interleaved in any order --
 * the [channels, time] buffer of a channelizer or network fan-in as it comes.  The objects they return are the
 * afsk_live / afsk_live_tx objects of this header: push, reset, info, submit, pull and destroy serve both kinds.
 *
 *  afsk_live_create_mixed   bit_frames_host: HOST array [n_channels], each as afsk_demod_batch_uniform
 *                           (AFSK_E_INVALID_BAUD); n_channels < 1 or a NULL array: AFSK_E_INVALID_ARG; the rest as
 *                           afsk_live_create (one pair of thresholds for all channels).  A burst of channel c is
 *                           demodulated at bit_frames_host[c] -- bit for bit what a uniform receiver of that rate reports
 *                           for the same channel.  Every entry equal: exactly afsk_live_create.  Otherwise the
 *                           receiver also owns a group plan over its n_channels * slots demodulator slots (slot
 *                           c * slots + k at bit_frames_host[c]; afsk_group_plan_create, 8 bytes per slot on the
 *                           device, which afsk_live_info adds to afsk_live_layout's bytes), and the push's second
 *                           launch is afsk_demod_batch_grouped over the slots -- still two launches, nothing on the
 *                           host in between, capturable.
 *  afsk_live_tx_create_mixed  bit_frames_host, ts_cycles_host: HOST arrays [n_channels]; each bit_frames a multiple of
 *                           4 in 4 ... 48000 (AFSK_E_INVALID_BAUD), each ts_cycles as afsk_live_tx_create, and every
 *                           channel's longest message bit_frames * (2 * ts_cycles + 4 + 14 * max_payload_len) + 4800 <=
 *                           AFSK_MAX_STREAM_LEN; n_channels < 1 or a NULL array: AFSK_E_INVALID_ARG.  Channel c plays
 *                           what a uniform transmitter of its geometry plays.  Every channel with the same bit_frames
 *                           and training length: exactly afsk_live_tx_create.  Otherwise the state is
 *                           afsk_live_tx_layout's plus int32 [n_channels, 2] (bit_frames, training symbols), which
 *                           afsk_live_tx_info reports.
 *  afsk_live_tx_state_bytes_mixed  host-only (no device needed): the state bytes of such a mixed transmitter
 *                           (afsk_live_tx_layout + the per-channel part, 256-byte aligned)
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_MIXED_SIGNATURES.)
 */
extern int afsk_live_create_mixed(int32_t n_channels, const int32_t *bit_frames_host, int32_t amp_start_threshold,
                                  int32_t amp_end_threshold, int32_t max_burst_len, int32_t max_chunk_len,
                                  afsk_live **out);

/*
 * The streaming live receiver (added after ABI version 2; the version is unchanged): the live receiver's gate, slots,
 * push, flush, reset and outputs, with every burst demodulated WHILE its blocks are gated.  It stores no samples of a
 * burst beyond the fewer than 4096 the next push needs, so a burst of any length is decoded and the state per channel
 * does not depend on burst length.  The object is an afsk_live: push, reset, info and destroy serve it unchanged.
 *
 *  afsk_live_stream_layout  host-only (no device needed): the slots per channel (1 + K / 3, as afsk_live_layout) and
 *                           the device state bytes afsk_live_create_stream would allocate:
 *                             a256(32 n) + a256(4096 n) + a256(32 n) + a256(4 n) + a256(8192 n)
 *                               + a256(max_payload_len * n) + 256,      a256(x) = x rounded up to a multiple of 256
 *                           (gate state, carry, demodulator, bit_frames, sample window, payload row), i.e. at most
 *                           16 KiB + max_payload_len + 256 bytes per channel, whatever the bursts' length.
 *  afsk_live_create_stream  bit_frames_host: HOST array [n_channels], each as afsk_demod_batch_uniform (a bad rate in
 *                           any channel: AFSK_E_INVALID_BAUD); amp_start / amp_end as afsk_live_create;
 *                           0 <= max_payload_len <= 65536 (the live transmitter's range), max_chunk_len as
 *                           afsk_live_create; n_channels < 1, a NULL array or NULL out: AFSK_E_INVALID_ARG.  Allocates
 *                           and zeroes the state on the current device (synchronous).
 * A push or flush of a streaming receiver gives, for any sequence of pushes:
 *   - the out_n_closed, out_burst_start, out_burst_len, out_flags and slot layout of a stored receiver whose
 *     max_burst_len holds every burst (AFSK_LIVE_OVERFLOW: see below);
 *   - for every used slot, the DemodOutputs (nbytes, nbits, clock_idx, term_frame, status, corrected, byte row) of
 *     afsk_demod_batch_uniform over the burst's recorded samples at its channel's bit_frames, except that a byte row
 *     holds at most min(max_payload_len, out_stride) bytes (nbytes still gives the full count);
 *   - unused slots written every push: length 0, flags 0, status AFSK_ST_TOO_SHORT, nbytes / nbits / corrected 0,
 *     clock_idx and term_frame -1;
 *   - AFSK_LIVE_OVERFLOW only for a burst longer than AFSK_MAX_STREAM_LEN, with status AFSK_ST_BAD_LENGTH (what the
 *     batch entries answer for that length) and burst_len saturating at 2^31 - 2048;
 *   - out_margins must be NULL (AFSK_E_INVALID_ARG otherwise); out_corrected is optional;
 *   - flush reports the open burst as AFSK_LIVE_OPEN_END, demodulated over its whole blocks; reset with a mask drops
 *     the masked channels' demodulator state too;
 *   - ONE launch on hip_stream, nothing on the host in between: capturable into a graph.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_STREAM_SIGNATURES.)
 */
extern int afsk_live_stream_layout(int32_t n_channels, int32_t max_payload_len, int32_t max_chunk_len,
                                   int32_t *out_slots, int64_t *out_state_bytes);
extern int afsk_live_create_stream(int32_t n_channels, const int32_t *bit_frames_host, int32_t amp_start_threshold,
                                   int32_t amp_end_threshold, int32_t max_payload_len, int32_t max_chunk_len,
                                   afsk_live **out);

/*
 * Live receivers with a gate and squelch threshold pair per channel (added after ABI version 2; the version is
 * unchanged).  Channel c gates with amp_start_host[c] / amp_end_host[c] and is demodulated with amp_end_host[c] at
 * bit_frames_host[c]: it reports, field for field, what a receiver of the same kind created with that one pair (and
 * rate) reports for its samples.  The objects are afsk_live: push, reset (which leaves the thresholds in place), info
 * and destroy serve them unchanged.
 *
 *  afsk_live_create_thresholds         the stored receiver (afsk_live_create_mixed's capacities and rates).
 *  afsk_live_create_stream_thresholds  the streaming receiver (afsk_live_create_stream's capacities and rates).
 *                           bit_frames_host, amp_start_host, amp_end_host: HOST int32 arrays [n_channels]; a NULL array,
 *                           NULL out or n_channels < 1: AFSK_E_INVALID_ARG, a bad rate AFSK_E_INVALID_BAUD, all
 *                           returned before any device is needed.  Every channel with the same pair: exactly the
 *                           receiver afsk_live_create_mixed / afsk_live_create_stream builds (its launches, its state
 *                           bytes).  Otherwise the state also holds amp_start and amp_end as int32 [n_channels] each
 *                           (afsk_live_info reports the larger state), and the gate reads a channel's pair once per push.
 * The streaming receiver's demodulator takes a channel's amp_end from the same array: any number of distinct values,
 * still one launch per push.  The stored receiver decodes with the batch demodulator, whose launches take one amp_end:
 * the channels are grouped by distinct amp_end into squelch classes, each with the list of its demodulator slots
 * c * slots + k on the device (int32 [n_channels * slots] in all; with mixed rates also every slot's bit_frames, another
 * int32 [n_channels * slots]), and a push is the gate launch plus ONE demod launch per class over that class's slots
 * -- every slot is in exactly one class, every output row is written once per push, nothing runs on the host in
 * between, so the push stays capturable.  amp_start may take any number of distinct values; distinct amp_end values
 * on a stored receiver are limited to AFSK_LIVE_MAX_SQUELCH_CLASSES (a push is at most 17 launches): more is
 * AFSK_E_INVALID_ARG (use the streaming receiver, which has no limit).  One class needs no list: the demod launch is
 * afsk_live_create_mixed's.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_THRESHOLD_SIGNATURES.)
 */
#define AFSK_LIVE_MAX_SQUELCH_CLASSES 16

extern int afsk_live_create_thresholds(int32_t n_channels, const int32_t *bit_frames_host, const int32_t *amp_start_host,
                                       const int32_t *amp_end_host, int32_t max_burst_len, int32_t max_chunk_len,
                                       afsk_live **out);
extern int afsk_live_create_stream_thresholds(int32_t n_channels, const int32_t *bit_frames_host,
                                              const int32_t *amp_start_host, const int32_t *amp_end_host,
                                              int32_t max_payload_len, int32_t max_chunk_len, afsk_live **out);

/*
 * Host-only (no device needed): the squelch classes afsk_live_create_thresholds would build for these channels and
 * `slots` slots per channel, for inspection and tests.  Classes in order of their first channel; out_slot_list
 * (int32 [n_channels * slots], optional) holds the classes' slot lists back to back, out_class_count their lengths,
 * out_class_uniform_bf the one bit_frames of a class's channels or 0 when they differ (arrays of
 * AFSK_LIVE_MAX_SQUELCH_CLASSES entries, optional).  *out_n_classes is the number of distinct amp_end values; above
 * the limit the call returns AFSK_E_INVALID_ARG with nothing else written.
 * (Declared `extern int`: bound from a table of its own, LIVE_CLASS_SIGNATURES.)
 */
extern int afsk_live_squelch_classes(int32_t n_channels, int32_t slots, const int32_t *bit_frames_host,
                                     const int32_t *amp_end_host, int32_t *out_n_classes, int32_t *out_class_amp_end,
                                     int32_t *out_class_count, int32_t *out_class_uniform_bf, int32_t *out_slot_list);

/*
 * The payload tap of the streaming live receiver (added after ABI version 2; the version is unchanged): a tapped push
 * also hands out, per channel, the payload bytes the demodulator committed DURING that push, with what it takes to
 * attribute each byte to its burst and to its offset in that burst's payload.  A byte decoded in the first second of a
 * long burst reaches the caller with the push that decoded it, not when the gate closes, and the tap never truncates:
 * with max_payload_len 0 a receiver keeps afsk_live_stream_layout's 16 KiB per channel and receives payloads of any
 * length.  A tapped receiver is an afsk_live with the state of afsk_live_create_stream_thresholds (afsk_live_stream_layout's
 * bytes, the thresholds behind them when they differ): info, reset and destroy serve it unchanged, and afsk_live_push
 * serves it as the streaming receiver it is -- such a push hands out nothing, its bytes are only in the payload rows.
 *
 *  afsk_live_tap_layout  host-only (no device needed): tap_cap, the bytes of one tap row -- an upper bound on what one
 *                        channel commits in one push, AFSK_LIVE_TAP_CAP(max_chunk_len, min_bit_frames) with
 *                        min_bit_frames the smallest bit_frames of the receiver:
 *                          ((K + 1) * 2048 / min_bit_frames) / 14 + 1,     K = (2047 + max_chunk_len) / 2048
 *                        (a push walks K blocks and may commit symbols of the one block before them, which waited for the
 *                        clock search: at most (K + 1) * 2048 / bf symbols; 14 symbols per byte; one byte more, begun in
 *                        an earlier push).  Refuses what afsk_live_stream_layout refuses (AFSK_E_INVALID_ARG) and a bad
 *                        min_bit_frames (AFSK_E_INVALID_BAUD).
 *  afsk_live_create_stream_tap  arguments, checks, state and gate of afsk_live_create_stream_thresholds; the receiver
 *                        also accepts afsk_live_push_tap.  Its tap_cap is afsk_live_tap_layout's for its smallest rate.
 *  afsk_live_push_tap    afsk_live_push (arguments, checks, outputs: field for field those of the untapped push) and,
 *                        DEVICE arrays written by every push:
 *                          tap_bytes    uint8 [n_channels, tap_cap]  the bytes committed during this push, in time order
 *                          tap_n        int32 [n_channels]           how many (<= tap_cap); the row beyond is not written
 *                          tap_len      int32 [n_channels, slots]    how many of them belong to the burst reported in
 *                                                                    slot (c, k) of this push; 0 for unused slots
 *                          open_start   int64 [n_channels]           first stream sample of the burst still recording
 *                                                                    after this push (its later out_burst_start), or -1
 *                          open_nbytes  int32 [n_channels]           payload bytes of that burst committed so far, this
 *                                                                    push's included; 0 when nothing is recording
 *                        A row reads [slot 0][slot 1] ... [open burst]: slot k's bytes start at the sum of tap_len[c, :k],
 *                        the open burst's share is tap_n - sum of tap_len[c, :n_closed].  For a burst reported with
 *                        nbytes = N, its bytes in the reporting push are payload bytes [N - tap_len, N), and its shares
 *                        of all pushes, in order, are the N bytes afsk_demod_batch_uniform decodes from its recorded
 *                        samples -- max_payload_len truncates the payload row, never the tap.  A burst that decodes
 *                        nothing hands out nothing.  A burst longer than AFSK_MAX_STREAM_LEN (AFSK_LIVE_OVERFLOW,
 *                        nbytes 0) reports tap_len 0; what earlier pushes handed out of it stays handed out.  After a
 *                        flush nothing is open (open_start -1).  A channel dropped by afsk_live_reset hands out nothing
 *                        more of its open burst, and its open_start is -1 until a new burst opens.  A receiver that was
 *                        not created by afsk_live_create_stream_tap: AFSK_E_INVALID_ARG.  ONE launch on hip_stream,
 *                        nothing on the host in between: capturable into a graph.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_TAP_SIGNATURES.)
 */
#define AFSK_LIVE_TAP_CAP(max_chunk_len, min_bit_frames) \
    ((int32_t)((((2047 + (int64_t)(max_chunk_len)) / 2048 + 1) * 2048 / (min_bit_frames)) / 14 + 1))

extern int afsk_live_tap_layout(int32_t n_channels, int32_t max_payload_len, int32_t max_chunk_len,
                                int32_t min_bit_frames, int32_t *out_tap_cap);
extern int afsk_live_create_stream_tap(int32_t n_channels, const int32_t *bit_frames_host, const int32_t *amp_start_host,
                                       const int32_t *amp_end_host, int32_t max_payload_len, int32_t max_chunk_len,
                                       afsk_live **out);
extern int afsk_live_push_tap(afsk_live *live, const int16_t *chunk, int64_t chunk_row_stride, int32_t chunk_len,
                              int32_t flush, int32_t *out_n_closed, int64_t *out_burst_start, int32_t *out_burst_len,
                              int32_t *out_flags, uint8_t *out_bytes, int32_t out_stride, int32_t *out_nbytes,
                              int32_t *out_nbits, int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                              int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride, uint8_t *tap_bytes,
                              int32_t *tap_n, int32_t *tap_len, int64_t *open_start, int32_t *open_nbytes,
                              void *hip_stream);

/*
 * The live transmitter (an addition: ABI version unchanged): Transmitter.transmit (:472-478) for n_channels
 * independent channels at one bit_frames and training length.  Every channel has a device-resident queue of up to
 * queue_depth messages; each pull writes the next n_samples samples of every channel's stream, the queued messages
 * back to back.  A channel's stream is what it produced since it was created or reset, numbered from 0; pos = samples
 * pulled so far.  A message of payload p is the .wav samples of Transmitter.save (:452-469 with the writer's
 * decimate/duplicate quirk :239-244): n_samples = bit_frames * (2 * ts_cycles + 4 + 14 * len(p)) + 4800.  Samples
 * outside any message are 0.  Submits and pulls never synchronise with the host; a pull of a fixed n_samples into a
 * fixed buffer can be captured into a graph.
 *
 *  afsk_live_tx_layout   host-only (no device needed): the device state bytes afsk_live_tx_create would allocate
 *  afsk_live_tx_create   bit_frames a multiple of 4 in 4 ... 48000 (the device modulator's symbol geometry; every rate a
 *                        Receiver decodes), else AFSK_E_INVALID_BAUD; ts_cycles as Transmitter (a negative value: no
 *                        training cycles); n_channels >= 1, 1 <= queue_depth <= 1024, 0 <= max_payload_len <= 65536,
 *                        n_channels * queue_depth < 2^31, the longest message <= AFSK_MAX_STREAM_LEN samples.
 *                        Allocates the state on the current device and zeroes it (synchronous).
 *  afsk_live_tx_info     n_channels, queue_depth, max_payload_len, state bytes; any pointer may be NULL
 *  afsk_live_tx_submit   queues n_msgs messages (DEVICE arrays): message i goes to channel[i], its payload is
 *                        payload_len[i] bytes at payload + payload_offset[i].  channel[] must be non-decreasing: from
 *                        the first message whose channel is below its predecessor's on, every message gets
 *                        AFSK_LIVE_TX_UNSORTED.  A channel's messages are queued in array order; a queued message
 *                        starts at max(pos, end of the channel's last queued message).  Rejected messages
 *                        (AFSK_LIVE_TX_QUEUE_FULL: queue_depth messages not yet fully emitted; _TOO_LONG: payload_len
 *                        outside 0 ... max_payload_len; _BAD_CHANNEL) take no queue entry.  Outputs (int32 status, int64
 *                        start = stream index of the first sample, int32 n_samples; -1 and 0 for a rejected message)
 *                        of message i go to entry out_index[i] (a permutation of 0 ... n_msgs - 1), or to entry i
 *                        when out_index is NULL.  The payload bytes are copied: the inputs may be reused once the
 *                        launches have run.  Two launches on hip_stream.
 *  afsk_live_tx_pull     writes samples [pos, pos + n_samples) of channel c to out + c * out_row_stride (samples,
 *                        2-byte alignment: a column window of a [channels, time] buffer works; out_row_stride >=
 *                        n_samples when n_channels > 1; out may be NULL when n_samples is 0) and nothing else of out,
 *                        then advances pos, retires the messages that have ended and writes out_pending[c] (int32
 *                        [n_channels]): the messages still queued or on air.  Two launches in order on hip_stream.
 *  afsk_live_tx_reset    drops every queued message (a half-sent one too) of every channel (d_mask_or_null NULL) or of
 *                        the channels whose DEVICE uint8 mask entry is non-zero: their streams restart at 0 and their
 *                        out_pending_or_null entries (when given) become 0
 *  afsk_live_tx_destroy  after the launches that use the transmitter have completed (NULL is fine)
 * Submits, pulls and resets of one transmitter must run in order (one stream, or ordered streams).
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_TX_SIGNATURES.)
 */
#define AFSK_LIVE_TX_QUEUED 0      /* accepted: start / n_samples are valid                                     */
#define AFSK_LIVE_TX_QUEUE_FULL 1  /* the channel already holds queue_depth messages not yet fully emitted       */
#define AFSK_LIVE_TX_TOO_LONG 2    /* payload_len outside 0 ... max_payload_len                                  */
#define AFSK_LIVE_TX_BAD_CHANNEL 3 /* channel outside 0 ... n_channels - 1                                      */
#define AFSK_LIVE_TX_UNSORTED 4    /* at or after the first message whose channel is below its predecessor's    */
typedef struct afsk_live_tx afsk_live_tx;
extern int afsk_live_tx_layout(int32_t n_channels, int32_t queue_depth, int32_t max_payload_len,
                               int64_t *out_state_bytes);
extern int afsk_live_tx_create(int32_t n_channels, int32_t bit_frames, int32_t ts_cycles, int32_t queue_depth,
                               int32_t max_payload_len, afsk_live_tx **out);
extern int afsk_live_tx_info(const afsk_live_tx *tx, int32_t *out_n_channels, int32_t *out_queue_depth,
                             int32_t *out_max_payload_len, int64_t *out_state_bytes);
extern int afsk_live_tx_submit(afsk_live_tx *tx, int32_t n_msgs, const int32_t *channel, const int64_t *payload_offset,
                               const int32_t *payload_len, const uint8_t *payload, const int32_t *out_index,
                               int32_t *out_status, int64_t *out_start, int32_t *out_n_samples, void *hip_stream);
extern int afsk_live_tx_pull(afsk_live_tx *tx, int16_t *out, int64_t out_row_stride, int32_t n_samples,
                             int32_t *out_pending, void *hip_stream);
extern int afsk_live_tx_reset(afsk_live_tx *tx, const uint8_t *d_mask_or_null, int32_t *out_pending_or_null,
                              void *hip_stream);
extern int afsk_live_tx_destroy(afsk_live_tx *tx);
/* per-channel rates: see afsk_live_create_mixed above */
extern int afsk_live_tx_create_mixed(int32_t n_channels, const int32_t *bit_frames_host, const int32_t *ts_cycles_host,
                                     int32_t queue_depth, int32_t max_payload_len, afsk_live_tx **out);
extern int afsk_live_tx_state_bytes_mixed(int32_t n_channels, int32_t queue_depth, int32_t max_payload_len,
                                          int64_t *out_state_bytes);

/*
 * Ragged pushes and pulls (added after ABI version 2; the version is unchanged): every channel of a live receiver or
 * transmitter takes its own number of samples per call, and every receiver channel has its own flush bit -- sources that
 * run on their own clocks, one source that disconnects while the others go on.  chunk_len / n_samples is the number of
 * COLUMNS of the buffer and bounds every channel's count; every host check of afsk_live_push / afsk_live_tx_pull
 * applies to it (max_chunk_len, the row stride, AFSK_MAX_STREAM_LEN).  The per-channel values are DEVICE arrays that
 * only the kernels read, never the host: a value below 0 counts as 0, a value above chunk_len / n_samples as
 * chunk_len / n_samples.  They are read when the launches RUN, so ONE captured graph of a fixed chunk_len / n_samples
 * serves ticks of any size up to it: rewrite the arrays (and the buffer) between replays.  The state is that of the
 * plain entries, and plain and ragged calls on one object may alternate.
 *
 *  afsk_live_push_ragged     afsk_live_push where channel c appends the first len_c = clamp(d_chunk_lens_or_null[c], 0,
 *                            chunk_len) samples of its row (int32 [n_channels]; NULL: chunk_len for every channel) and
 *                            its stream ends when flush != 0 or d_flush_mask_or_null[c] != 0 (uint8 [n_channels]; NULL:
 *                            flush alone decides).  No sample at or beyond column len_c of a row is read.  A channel that
 *                            is flushed reports its open burst (AFSK_LIVE_OPEN_END), drops its partial block and starts
 *                            a new stream at sample 0; the others are not touched by it.  A channel with len_c = 0 and no
 *                            flush keeps its state exactly -- carry, gate mode, open burst, streaming window -- and
 *                            reports n_closed 0 (and with the tap outputs tap_n 0, open_start / open_nbytes of the burst
 *                            still open).  Outputs: every output of afsk_live_push_tap, in its order.  The five tap
 *                            pointers are all NULL or all given (some of them: AFSK_E_INVALID_ARG).  All NULL: the
 *                            untapped push, also on a tapped receiver (as afsk_live_push there).  All given: the tapped
 *                            push; a receiver that was not created by afsk_live_create_stream_tap: AFSK_E_INVALID_ARG.
 *                            The launches are afsk_live_push's: two for a stored receiver (one more per further squelch
 *                            class), ONE for a streaming or tapped one, nothing on the host in between: capturable into a
 *                            graph.
 *  afsk_live_tx_pull_ragged  afsk_live_tx_pull where channel c writes samples [pos_c, pos_c + len_c) to columns
 *                            [0, len_c) of its row, len_c = clamp(d_lens_or_null[c], 0, n_samples) (int32 [n_channels];
 *                            NULL: n_samples for every channel), writes nothing to columns [len_c, n_samples), then
 *                            advances pos_c by len_c, retires the messages that have ended by then and writes
 *                            out_pending[c].  Two launches in order on hip_stream, capturable into a graph.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_RAGGED_SIGNATURES.)
 */
extern int afsk_live_push_ragged(afsk_live *live, const int16_t *chunk, int64_t chunk_row_stride, int32_t chunk_len,
                                 const int32_t *d_chunk_lens_or_null, int32_t flush, const uint8_t *d_flush_mask_or_null,
                                 int32_t *out_n_closed, int64_t *out_burst_start, int32_t *out_burst_len,
                                 int32_t *out_flags, uint8_t *out_bytes, int32_t out_stride, int32_t *out_nbytes,
                                 int32_t *out_nbits, int32_t *out_clock_idx, int32_t *out_term_frame,
                                 int32_t *out_status, int32_t *out_corrected, int32_t *out_margins,
                                 int32_t margin_stride, uint8_t *tap_bytes, int32_t *tap_n, int32_t *tap_len,
                                 int64_t *open_start, int32_t *open_nbytes, void *hip_stream);
extern int afsk_live_tx_pull_ragged(afsk_live_tx *tx, int16_t *out, int64_t out_row_stride, int32_t n_samples,
                                    const int32_t *d_lens_or_null, int32_t *out_pending, void *hip_stream);

/*
 * The packed event list of a push (added after ABI version 2; the version is unchanged).  A push answers in slots:
 * finding the handful of bursts it closed means copying n_closed, the slot arrays and every payload row of every channel.
 * afsk_live_pack turns the outputs of ONE push -- of any receiver kind and of the plain, tapped or ragged entry alike --
 * into a compact list on the device, so that the host copies a 32-byte header, `stored` records and `stored_bytes`
 * payload bytes: a cost in proportion to what closed.  It reads the push's outputs and writes only into the events
 * buffer, one caller-provided DEVICE allocation of out_total_bytes, 16-byte aligned:
 *
 *   [0, 32)                                  the header
 *        int32 count         bursts the push reported, over all channels (the sum of n_closed); may exceed max_events
 *        int32 stored        min(count, max_events): the records written
 *        int64 n_bytes       kept payload bytes of all `count` bursts
 *        int64 stored_bytes  payload bytes actually written
 *        8 bytes reserved, written as 0
 *   [records_offset, + 48 * max_events)      afsk_live_event records (records_offset = 32)
 *   [payload_offset, + max_bytes)            the records' payloads back to back in record order
 *   [.., out_total_bytes)                    scratch of the scan: 16 bytes per AFSK_LIVE_EVENTS_SPAN channels
 *
 * Record order is channel ascending, then slot ascending -- the order in which a host loop over n_closed visits the
 * slots -- and is the same on every replay.  A record holds the slot's values as the slot arrays hold them:
 *
 *   offset  0  int32 channel
 *           4  int32 slot            k: the record is slot (channel, k), demodulator row channel * slots + k
 *           8  int64 burst_start
 *          16  int32 burst_len
 *          20  int32 flags           AFSK_LIVE_OPEN_END | AFSK_LIVE_OVERFLOW
 *          24  int32 status
 *          28  int32 nbytes          the demodulator's full count (a truncated streaming row: above out_stride)
 *          32  int32 nbits
 *          36  int32 clock_idx
 *          40  int32 term_frame
 *          44  int32 payload_offset  where its payload starts in the payload part, or -1: not written
 *
 * A record keeps kept = min(max(nbytes, 0), out_stride) bytes of its row, and 0 with AFSK_LIVE_OVERFLOW.  Its
 * payload_offset is the sum of the kept bytes of ALL records before it, and -1 when that sum + kept exceeds max_bytes:
 * that payload is not written.  Records from index max_events on are not written, nor are their payloads; the header
 * still holds the true count and n_bytes, so the host sees that the list is short and reads the slot arrays.  Nothing is
 * written outside the header, the first `stored` records, the first stored_bytes payload bytes and the scratch.
 * Only n_closed is read for every channel: the slot arrays and the rows are read for slots k < n_closed[c] alone.
 * Channel c reports clamp(n_closed[c], 0, slots) bursts: a value outside [0, slots] counts as the nearer end, in count
 * and in the records alike.  On the outputs of a real push the clamp changes nothing.
 *
 *  afsk_live_events_layout  host-only, needs no device: the offsets of the records and of the payload part and the size
 *                           of the events buffer for max_events records and max_bytes payload bytes
 *                           (records_offset = 32, payload_offset = 32 + 48 * max_events, out_total_bytes = payload_offset
 *                           + max_bytes rounded up to 16, + 16 * AFSK_LIVE_EVENTS_BLOCKS(n_channels)).
 *                           n_channels * slots records and that many times out_stride bytes never overflow.
 *  afsk_live_pack           packs the outputs of one push: n_closed [n_channels]; burst_start, burst_len, flags
 *                           [n_channels, slots]; out_bytes [n_channels * slots, out_stride] (may be NULL when out_stride
 *                           is 0); nbytes, nbits, clock_idx, term_frame, status [n_channels * slots] -- all DEVICE
 *                           pointers, as the push wrote them.  It takes no receiver: it is a function of the arrays.
 *                           Three launches in order on hip_stream (totals per span of channels, one block's scan of
 *                           those totals, records and payloads); no block waits for another.  No allocation, no
 *                           synchronisation, no host read: capturable into a graph behind the push.
 * Both: AFSK_E_INVALID_ARG for n_channels < 1, slots < 1, n_channels * slots >= 2^31, max_events < 0, max_bytes < 0 or
 * >= 2^31, or a NULL pointer.  afsk_live_pack alone: AFSK_E_INVALID_ARG also for out_stride < 0 and for an events buffer
 * that is not 16-byte aligned (the records and the payload copy are written with 16-byte stores), and AFSK_E_NO_DEVICE
 * without a device.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_EVENT_SIGNATURES.)
 */
#define AFSK_LIVE_EVENTS_SPAN 256 /* channels one block of the pack kernels scans */
#define AFSK_LIVE_EVENTS_BLOCKS(n_channels) (((int64_t)(n_channels) + AFSK_LIVE_EVENTS_SPAN - 1) / AFSK_LIVE_EVENTS_SPAN)
typedef struct afsk_live_event {
    int32_t channel;
    int32_t slot;
    int64_t burst_start;
    int32_t burst_len;
    int32_t flags;
    int32_t status;
    int32_t nbytes;
    int32_t nbits;
    int32_t clock_idx;
    int32_t term_frame;
    int32_t payload_offset;
} afsk_live_event;
extern int afsk_live_events_layout(int32_t n_channels, int32_t slots, int32_t max_events, int64_t max_bytes,
                                   int64_t *out_records_offset, int64_t *out_payload_offset, int64_t *out_total_bytes);
extern int afsk_live_pack(int32_t n_channels, int32_t slots, const int32_t *n_closed, const int64_t *burst_start,
                          const int32_t *burst_len, const int32_t *flags, const uint8_t *out_bytes, int32_t out_stride,
                          const int32_t *nbytes, const int32_t *nbits, const int32_t *clock_idx,
                          const int32_t *term_frame, const int32_t *status, void *events, int32_t max_events,
                          int64_t max_bytes, void *hip_stream);

/*
 * The packed segment list of a progressive push (added after ABI version 2; the version is unchanged).  The payload tap
 * answers in whole arrays too: reading what one push decoded means copying tap_bytes, tap_n, tap_len, open_start and
 * open_nbytes of every channel.  afsk_live_pack_tap turns the outputs of ONE tapped push (afsk_live_push_tap, or
 * afsk_live_push_ragged with the tap pointers given) into a compact list on the device, so that the host copies a
 * 32-byte header, `stored` records and `stored_bytes` data bytes: a cost in proportion to what decoded.  It reads the
 * push's outputs and writes only into the segments buffer, one caller-provided DEVICE allocation of out_total_bytes,
 * 16-byte aligned:
 *
 *   [0, 32)                                  the header of the events buffer, field for field
 *        int32 count         segments of the push, over all channels; may exceed max_segments (exact while
 *                            n_channels * (slots + 1) < 2^31, held at 2^31 - 1 beyond)
 *        int32 stored        min(count, max_segments): the records written
 *        int64 n_bytes       data bytes of all `count` segments
 *        int64 stored_bytes  data bytes actually written
 *        8 bytes reserved, written as 0
 *   [records_offset, + 32 * max_segments)    afsk_live_segment records (records_offset = 32)
 *   [data_offset, + max_bytes)               the records' data back to back in record order
 *   [.., out_total_bytes)                    scratch of the scan: 16 bytes per AFSK_LIVE_EVENTS_SPAN channels
 *
 * The per-channel rule.  For channel c: nc = clamp(n_closed[c], 0, slots) and tn = clamp(tap_n[c], 0, tap_cap); with
 * at = 0, every slot k < nc in turn takes ln_k = clamp(tap_len[c, k], 0, tn - at) bytes and at += ln_k; rest = tn - at.
 * The channel has an OPEN segment iff rest > 0 and open_start[c] >= 0.  It contributes nc FINAL records -- one per burst
 * the push reported, with length 0 where the burst closed without new bytes -- and then the open record if it has one:
 *
 *   offset  0  int32 channel       c
 *           4  int32 slot          k: a final segment, of slot (c, k); -1: the open segment
 *           8  int64 burst_start   burst_start[c, k]                  open: open_start[c]
 *          16  int32 burst_len     burst_len[c, k]                    open: 0
 *          20  int32 flags         flags[c, k]                        open: 0
 *          24  int32 offset        nbytes[c * slots + k] - ln_k       open: open_nbytes[c] - rest
 *                                  (where in the burst's payload the data belong)
 *          28  int32 length        ln_k                               open: rest
 *
 * Its data are tap_bytes[c, 0 : at] and, with an open segment, [at : at + rest]: one contiguous run of the tap row that
 * lands as one contiguous run of the data part.  On the outputs of a real push the clamps change nothing.
 *
 * Record order is channel ascending, then the slots ascending, then the open segment, and is the same on every replay.
 * The data lie back to back in record order; a record holds no data offset: its data start at the sum of the lengths of
 * all records before it.  A record's data are written iff the record is stored (its index is below max_segments) and its
 * start plus its length is at most max_bytes; stored_bytes is the start of the first record whose data are not written,
 * or n_bytes when all are.  The header always holds the true count and n_bytes, so the host sees that the list is short
 * and reads the tap arrays.  Nothing is written outside the header, the first `stored` records, the first stored_bytes
 * data bytes and the scratch, also when a channel's run straddles max_bytes.  n_channels * (slots + 1) records and
 * n_channels * tap_cap bytes never overflow.  For every channel only n_closed and tap_n are read; tap_len for k < nc
 * alone; open_start and open_nbytes only where rest > 0; the slot arrays and the tap rows only for what is written.
 *
 *  afsk_live_segments_layout  host-only, needs no device: the offsets of the records and of the data part and the size
 *                             of the segments buffer (records_offset = 32, data_offset = 32 + 32 * max_segments,
 *                             out_total_bytes = data_offset + max_bytes rounded up to 16,
 *                             + 16 * AFSK_LIVE_EVENTS_BLOCKS(n_channels)).
 *  afsk_live_pack_tap         packs the outputs of one tapped push: n_closed [n_channels]; burst_start, burst_len, flags
 *                             [n_channels, slots]; nbytes [n_channels * slots]; tap_bytes [n_channels, tap_cap]; tap_n
 *                             [n_channels]; tap_len [n_channels, slots]; open_start, open_nbytes [n_channels] -- all
 *                             DEVICE pointers, as the push wrote them.  It takes no receiver: it is a function of the
 *                             arrays.  Three launches in order on hip_stream (totals per span of channels, one block's
 *                             scan of those totals, then a thread per channel writes its records and copies its bytes);
 *                             no block waits for another.  No allocation, no synchronisation, no host read: capturable
 *                             into a graph behind the push.
 * Both: AFSK_E_INVALID_ARG for what afsk_live_events_layout refuses (max_segments in the place of max_events) or a NULL
 * pointer.  afsk_live_pack_tap alone: AFSK_E_INVALID_ARG also for tap_cap < 1 and for a segments buffer that is not
 * 16-byte aligned (the records are written with 16-byte stores), and AFSK_E_NO_DEVICE without a device.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_SEGMENT_SIGNATURES.)
 */
typedef struct afsk_live_segment {
    int32_t channel;
    int32_t slot;
    int64_t burst_start;
    int32_t burst_len;
    int32_t flags;
    int32_t offset;
    int32_t length;
} afsk_live_segment;
extern int afsk_live_segments_layout(int32_t n_channels, int32_t slots, int32_t max_segments, int64_t max_bytes,
                                     int64_t *out_records_offset, int64_t *out_data_offset, int64_t *out_total_bytes);
extern int afsk_live_pack_tap(int32_t n_channels, int32_t slots, int32_t tap_cap, const int32_t *n_closed,
                              const int64_t *burst_start, const int32_t *burst_len, const int32_t *flags,
                              const int32_t *nbytes, const uint8_t *tap_bytes, const int32_t *tap_n,
                              const int32_t *tap_len, const int64_t *open_start, const int32_t *open_nbytes,
                              void *segments, int32_t max_segments, int64_t max_bytes, void *hip_stream);

/*
 * Rate detection (an addition, no reference counterpart: the reference's Receiver is told its baud rate): which of
 * n_cand candidate bit_frames values each stream was sent at, decided on the device from the stream's first
 * AFSK_SYNC_WINDOW samples, so that out_bit_frames feeds the bit_frames argument of afsk_demod_batch / _ex directly --
 * both launches on one stream, nothing copied to the host in between.
 *
 * For a stream with stream_len[s] >= 4096, x = its first 4096 raw samples, and a candidate bf with tc = the training
 * cycle of that rate (mark ++ space, 2 bf samples, :88-91), all in integers:
 *   total(i) = sum_{j < 2bf} |tc[j] - x[i + j]|       for i in [0, 4096 - 2bf)   (the sums of :327-331)
 *   d(i)     = total(i) / (2bf);  ci(bf) = the first i with minimal d(i)         (the Receiver's clock index, :332-337)
 *   n        = (4096 - 2bf - 1 - ci) / (2bf) + 1                                 (the whole cycles at ci, ci + 2bf, ...
 *                                                                                 that start inside the search range)
 *   score(bf) = (sum_{k < n} total(ci + k 2bf)) / (n 2bf)                        (0 ... 65535: the mean absolute
 *                                                                                 difference per sample over them)
 * The detected rate is the candidate of smallest score; on a tie the earliest position of the list wins (so duplicate
 * candidates are legal).  The minimum d(ci) of ONE cycle is not enough: a short window (8 samples at bf = 4) matches
 * noise somewhere among 4088 offsets.  Candidates with bf >= 1200 (below 48 baud) are legal but not reliably told
 * apart: at most one or two of their cycles fit the window.
 *
 *  cand_bit_frames_host  [n_cand] HOST array, copied into the launch arguments before the call returns (no upload, no
 *                        allocation: the launch captures into a graph); 1 <= n_cand <= AFSK_DETECT_MAX_CANDIDATES
 *  out_bit_frames   [n] the detected candidate; 0 for a stream that is not examined
 *  out_score        [n] its score; -1 for such a stream
 *  out_runner_up    [n] the smallest score among the OTHER positions of the list; -1 with one candidate or for such a
 *                       stream
 *  out_clock_idx    [n] ci of the detected candidate; -1 for such a stream
 *  out_scores       [n, n_cand] every candidate's score (-1 for such a stream), or NULL
 * A stream shorter than 4096 samples, or of a length outside 0 ... AFSK_MAX_STREAM_LEN, is not examined and nothing of
 * it is read; afsk_demod_batch answers its bit_frames of 0 with AFSK_ST_INVALID_BAUD and no bytes.  Streams may start
 * at any sample offset, as for afsk_demod_batch.  All arrays but the candidates are DEVICE pointers.
 *
 * One launch, a workgroup per stream (afsk_detect.hip), asynchronous on hip_stream.  AFSK_E_INVALID_ARG for n_cand
 * outside 1 ... 36, a negative n_streams or a NULL pointer (out_scores excepted); AFSK_E_INVALID_BAUD for a candidate
 * afsk_demod_batch_uniform would refuse; n_streams == 0 returns AFSK_OK without a launch; AFSK_E_NO_DEVICE without a
 * device.  (Declared `extern int`: afskmodem_amd/_native.py binds it from a table of its own, DETECT_SIGNATURES.)
 */
#define AFSK_DETECT_MAX_CANDIDATES 36 /* every bit_frames value with a Receiver: the multiples of 4 below 2048 that divide 48000 */
extern int afsk_detect_rate_batch(const int16_t *samples, const int64_t *stream_offset, const int32_t *stream_len,
                                  int32_t n_streams, const int32_t *cand_bit_frames_host, int32_t n_cand,
                                  int32_t *out_bit_frames, int32_t *out_score, int32_t *out_runner_up,
                                  int32_t *out_clock_idx, int32_t *out_scores /* [n, n_cand] or NULL */,
                                  void *hip_stream);

/*
 * The auto-rate streaming live receiver (an addition: ABI version unchanged): a streaming receiver
 * (afsk_live_create_stream_thresholds) whose channels have no rate of their own.  The rate is decided per BURST, on the
 * device, inside the push that records the burst's second block: over the burst's first 4096 samples every candidate's
 * (ci, score) is computed exactly as defined for afsk_detect_rate_batch above, the smallest score wins and the earliest
 * list position wins a tie.  From then on the burst is what a fixed-rate streaming receiver of the winner's rate makes of
 * it: clock index = the winner's ci, the per-symbol squelch from the channel's amp_end and that rate, the same terminator
 * search, squelch stop, Hamming decode, payload row, truncation at max_payload_len and tap.  A channel's successive
 * bursts may have any rates in any order.  The open burst's rate is part of the channel's state: it survives across
 * pushes and is cleared where the open burst is dropped (afsk_live_reset, masked or not).
 *
 *  afsk_live_create_stream_auto  cand_bit_frames_host: [n_cand] HOST array, 1 <= n_cand <= AFSK_DETECT_MAX_CANDIDATES,
 *                        each a bit_frames afsk_demod_batch_uniform accepts (else AFSK_E_INVALID_BAUD); duplicates are
 *                        legal; candidates with bf >= 1200 are accepted and unreliable, as for the detector.  max_score
 *                        >= 0: a burst whose best score exceeds it is not demodulated (below); < 0: none.  amp_start_host
 *                        / amp_end_host: [n_channels] each, as afsk_live_create_stream_thresholds (one pair for all
 *                        channels: the shared-pair receiver).  tap = 1: with the payload tap of
 *                        afsk_live_create_stream_tap, its tap_cap = AFSK_LIVE_TAP_CAP(max_chunk_len, the smallest
 *                        candidate); tap = 0: without.  State, slots and limits: afsk_live_stream_layout's.
 *  afsk_live_push_auto   afsk_live_push_ragged's arguments, checks and outputs, and in front of hip_stream two more
 *                        DEVICE arrays, int32 [n_channels * slots], written by every push:
 *                          out_bit_frames   the burst's detected bit_frames; 0 for an unused slot, for a burst reported
 *                                           with fewer than 4096 samples (status AFSK_ST_TOO_SHORT, as on every
 *                                           receiver) and for a burst refused by max_score
 *                          out_rate_score   the winner's score; -1 for an unused slot and for such a short burst
 *                        A burst refused by max_score reports status AFSK_ST_INVALID_BAUD, nbytes = nbits = 0,
 *                        clock_idx = term_frame = -1, out_bit_frames 0 and its score, and hands out no tap bytes.
 *                        NULL lengths and a NULL mask launch the plain cells.  The five tap outputs are all NULL or all
 *                        given; given needs tap = 1.  ONE launch on hip_stream, no allocation, no synchronisation:
 *                        capturable into a graph.  With ONE candidate r every output equals, bit for bit, that of the
 *                        fixed-rate streaming receiver at r.
 * afsk_live_push, afsk_live_push_tap and afsk_live_push_ragged refuse an auto-rate receiver and afsk_live_push_auto
 * refuses every other one (AFSK_E_INVALID_ARG; afsk_last_error names the right entry).  afsk_live_info, afsk_live_reset,
 * afsk_live_destroy, afsk_live_pack and afsk_live_pack_tap serve it unchanged.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_AUTO_SIGNATURES.)
 */
extern int afsk_live_create_stream_auto(int32_t n_channels, const int32_t *cand_bit_frames_host, int32_t n_cand,
                                        int32_t max_score /* < 0: none */, const int32_t *amp_start_host,
                                        const int32_t *amp_end_host, int32_t max_payload_len, int32_t max_chunk_len,
                                        int32_t tap /* 0 / 1 */, afsk_live **out);
extern int afsk_live_push_auto(afsk_live *live, const int16_t *chunk, int64_t chunk_row_stride, int32_t chunk_len,
                               const int32_t *d_chunk_lens_or_null, int32_t flush, const uint8_t *d_flush_mask_or_null,
                               int32_t *out_n_closed, int64_t *out_burst_start, int32_t *out_burst_len,
                               int32_t *out_flags, uint8_t *out_bytes, int32_t out_stride, int32_t *out_nbytes,
                               int32_t *out_nbits, int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                               int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride, uint8_t *tap_bytes,
                               int32_t *tap_n, int32_t *tap_len, int64_t *open_start, int32_t *open_nbytes,
                               int32_t *out_bit_frames, int32_t *out_rate_score, void *hip_stream);

/*
 * The relay submit of the live transmitter (added after ABI version 2; the version is unchanged): a station that
 * answers what it hears -- a digipeater, a cross-rate gateway, a many-channel repeater -- queues the bursts a push closed
 * on a live transmitter straight from the packed event list afsk_live_pack left on the device.  Nothing goes through the
 * host, so push + pack + submit + pull is one capturable chain of launches.
 *
 *  afsk_live_relay_check_map   host-only (no device needed).  map_host: HOST int32 [n_rx_channels]; entry c is the
 *                              transmitter channel the bursts of receiver channel c go to.  A negative entry: channel c
 *                              is not relayed.  An entry >= n_tx_channels is allowed (its records are answered with
 *                              AFSK_LIVE_TX_BAD_CHANNEL).  Two receiver channels that name the same transmitter channel
 *                              in 0 ... n_tx_channels - 1: AFSK_E_INVALID_ARG, afsk_last_error names both (the submit
 *                              gives every destination channel to ONE wave; an ordering rule across receiver channels
 *                              does not exist).  A NULL map is the identity: AFSK_OK.  n_rx_channels < 1 or
 *                              n_tx_channels < 1: AFSK_E_INVALID_ARG.
 *  afsk_live_tx_submit_events  events: a DEVICE events buffer as afsk_live_pack wrote it, with the offsets of
 *                              afsk_live_events_layout for these max_events / max_bytes; out_stride: that push's;
 *                              n_rx_channels: the receiver's channels; d_channel_map_or_null: DEVICE int32
 *                              [n_rx_channels] (a map afsk_live_relay_check_map accepts) or NULL, the identity.  The
 *                              three outputs are DEVICE arrays of max_events entries, all written by every call.
 *                              `stored` is read on the device and clamped to 0 ... max_events.  Record i, in this order:
 *                                1. i >= stored: AFSK_LIVE_TX_NONE, start -1, n_samples 0
 *                                2. at or after the first stored record whose channel is below its predecessor's:
 *                                   AFSK_LIVE_TX_UNSORTED (afsk_live_tx_submit's guard; a real pack never trips it)
 *                                3. not relayable: AFSK_LIVE_TX_SKIPPED -- flags & (AFSK_LIVE_OVERFLOW | skip_flags),
 *                                   status != AFSK_ST_OK, nbytes < 1, nbytes > out_stride (a truncated streaming row),
 *                                   payload_offset < 0 or payload_offset + nbytes > max_bytes
 *                                4. the destination: the record's channel without a map.  With a map a record channel
 *                                   outside 0 ... n_rx_channels - 1 gets AFSK_LIVE_TX_BAD_CHANNEL (the map is not read
 *                                   for it), else dst = map[channel]: negative AFSK_LIVE_TX_SKIPPED, >= the
 *                                   transmitter's channels AFSK_LIVE_TX_BAD_CHANNEL
 *                                5. afsk_live_tx_submit's rules and outputs on channel dst with the record's nbytes
 *                                   payload bytes: _TOO_LONG, _QUEUE_FULL, or _QUEUED with start = max(pos, end) and
 *                                   n_samples from dst's geometry (uniform and mixed transmitters alike)
 *                              A destination channel's records are queued in record order; the state afterwards is what
 *                              afsk_live_tx_submit leaves when given the relayable records' destinations and payloads
 *                              in that order.  skip_flags: AFSK_LIVE_OPEN_END skips a burst a flush reported while it
 *                              was still recording (its payload may be cut short), 0 relays it.  Reads the header, the
 *                              first `stored` records, the payload bytes of queued records and the map; writes nothing
 *                              of the events buffer; whatever the header and the records hold, no access leaves the
 *                              buffers given (a payload range outside [0, max_bytes) is skipped, not read).  At most
 *                              two launches in order on hip_stream, no allocation, no synchronisation, no host read of
 *                              a device value: capturable behind push and pack.  AFSK_E_INVALID_ARG, nothing launched:
 *                              a NULL tx, events or output; max_events, max_bytes or out_stride < 0; n_rx_channels < 1;
 *                              skip_flags with bits other than AFSK_LIVE_OPEN_END | AFSK_LIVE_OVERFLOW; an events
 *                              pointer that is not 16-byte aligned.  max_events == 0: AFSK_OK, no launch.
 * Submits of both kinds, pulls and resets of one transmitter must run in order.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_RELAY_SIGNATURES.)
 */
#define AFSK_LIVE_TX_SKIPPED 5 /* afsk_live_tx_submit_events: the record is not relayable or its channel is not mapped */
#define AFSK_LIVE_TX_NONE (-1) /* afsk_live_tx_submit_events: the entry is at or past `stored`: no record            */
extern int afsk_live_relay_check_map(const int32_t *map_host, int32_t n_rx_channels, int32_t n_tx_channels);
extern int afsk_live_tx_submit_events(afsk_live_tx *tx, const void *events, int32_t max_events, int32_t max_bytes,
                                      int32_t out_stride, int32_t n_rx_channels, const int32_t *d_channel_map_or_null,
                                      int32_t skip_flags, int32_t *out_status, int64_t *out_start,
                                      int32_t *out_n_samples, void *hip_stream);

/*
 * The rated live transmitter (added after ABI version 2; the version is unchanged): a rate per queued MESSAGE, where
 * afsk_live_tx_create has one for the transmitter's life and afsk_live_tx_create_mixed one per channel -- a digipeater
 * on a shared calling channel repeats every burst at the rate it heard.  The transmitter holds a table of up to
 * AFSK_DETECT_MAX_CANDIDATES geometries and every queued message names one entry; queues, back-to-back starts, pulls
 * (plain and ragged), pending, reset, info and destroy are afsk_live_tx's own.
 *
 *  afsk_live_tx_state_bytes_rated  host-only (no device needed): the state bytes of such a transmitter --
 *                              afsk_live_tx_layout's, then the table int32 [n_rates, 2] (bit_frames, training symbols),
 *                              then int32 [n_channels, queue_depth, 2], the geometry of every ring entry; each part
 *                              256-byte aligned.  afsk_live_tx_info reports the same total.
 *  afsk_live_tx_create_rated   Transmitter.__init__ (ref:436-450) once per table entry: bit_frames_host, ts_cycles_host
 *                              HOST arrays [n_rates], n_rates in 1 ... 36 (AFSK_E_INVALID_ARG), each bit_frames a
 *                              multiple of 4 in 4 ... 48000 (AFSK_E_INVALID_BAUD), each ts_cycles as afsk_live_tx_create
 *                              (negative: no training cycles, ref:457), and every entry's longest message at most
 *                              AFSK_MAX_STREAM_LEN samples.  Equal bit_frames in two entries are fine (two training
 *                              lengths at one rate).  The arrays are the caller's again on return.
 *  afsk_live_tx_submit_rated   afsk_live_tx_submit (Transmitter.transmit's samples, ref:452-469 and 472-478, queued)
 *                              with rate_index: DEVICE int32 [n_msgs], the table entry message i plays at, or NULL:
 *                              entry 0 for all.  n_samples = bit_frames * (2 * ts_cycles + 4 + 14 * payload_len) + 4800
 *                              of that entry.  An index outside 0 ... n_rates - 1: AFSK_LIVE_TX_BAD_RATE, nothing
 *                              queued.  The checks of a message run in this order: _UNSORTED, _BAD_CHANNEL, _TOO_LONG,
 *                              _BAD_RATE, _QUEUE_FULL.  Two launches, as afsk_live_tx_submit.
 *  afsk_live_tx_submit_events_rated  afsk_live_tx_submit_events (ref:472-478 for every burst heard) with the rate of
 *                              record r read on the device from d_rx_bit_frames[r.channel * rx_slots + r.slot]: the
 *                              DEVICE int32 [n_rx_channels, rx_slots] array afsk_live_push_auto wrote as
 *                              out_bit_frames in the push the events were packed from.  The first table entry with that
 *                              bit_frames is the message's; none (a burst the receiver did not rate holds 0):
 *                              AFSK_LIVE_TX_BAD_RATE.  A record whose channel lies outside 0 ... n_rx_channels - 1 or
 *                              whose slot lies outside 0 ... rx_slots - 1 is AFSK_LIVE_TX_SKIPPED and the array is not
 *                              read for it.  Order: afsk_live_tx_submit_events' steps 1 - 3 with that condition among
 *                              the _SKIPPED ones (so a record that is not relayable never reads the array), then
 *                              _BAD_CHANNEL, _TOO_LONG, _BAD_RATE, _QUEUE_FULL.  Two launches, no atomics, no host read.
 *                              AFSK_E_INVALID_ARG besides afsk_live_tx_submit_events': a NULL d_rx_bit_frames,
 *                              rx_slots < 1.
 * On a rated transmitter afsk_live_tx_submit and afsk_live_tx_submit_events queue every message at table entry 0.  The
 * two _rated submit entries on a transmitter that is not rated: AFSK_E_INVALID_ARG, nothing launched.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_TX_RATED_SIGNATURES.)
 */
#define AFSK_LIVE_TX_BAD_RATE 6 /* rate_index outside the table / the rate heard is not in the table: nothing queued */
extern int afsk_live_tx_state_bytes_rated(int32_t n_channels, int32_t n_rates, int32_t queue_depth,
                                          int32_t max_payload_len, int64_t *out_state_bytes);
extern int afsk_live_tx_create_rated(int32_t n_channels, int32_t n_rates, const int32_t *bit_frames_host,
                                     const int32_t *ts_cycles_host, int32_t queue_depth, int32_t max_payload_len,
                                     afsk_live_tx **out);
extern int afsk_live_tx_submit_rated(afsk_live_tx *tx, int32_t n_msgs, const int32_t *channel,
                                     const int32_t *rate_index, const int64_t *payload_offset,
                                     const int32_t *payload_len, const uint8_t *payload, const int32_t *out_index,
                                     int32_t *out_status, int64_t *out_start, int32_t *out_n_samples, void *hip_stream);
extern int afsk_live_tx_submit_events_rated(afsk_live_tx *tx, const void *events, int32_t max_events,
                                            int32_t max_bytes, int32_t out_stride, int32_t n_rx_channels,
                                            const int32_t *d_channel_map_or_null, int32_t skip_flags,
                                            const int32_t *d_rx_bit_frames, int32_t rx_slots, int32_t *out_status,
                                            int64_t *out_start, int32_t *out_n_samples, void *hip_stream);

/*
 * Carrier sense (added after ABI version 2; the version is unchanged): a transmitter channel stays off the air while
 * the receiver of that channel is hearing a burst, and for a slot time after it stops -- what a packet-radio TNC does
 * with data carrier detect.  Both halves run on the device, so push -> busy -> submit_events -> pull is one captured
 * graph with no host read in it.  All of it is integer and sample-exact.
 *
 *  afsk_live_busy          d_out_busy[c] (DEVICE int32 [n_channels]) = 1 when channel c's gate is recording a burst (it
 *                          has heard a block above amp_start and none below amp_end since), else 0: the state the
 *                          last push, flush or reset left, for a receiver of any kind (stored, streaming, tapped, auto;
 *                          one rate or mixed; one threshold pair or one per channel; plain or ragged pushes).  One
 *                          launch of one thread per channel on hip_stream, after the pushes it is ordered behind.
 *  afsk_live_tx_pull_hold  afsk_live_tx_pull_ragged (its arguments, its checks, d_lens_or_null NULL: n_samples for every
 *                          channel) with d_hold_or_null (DEVICE int32 [n_channels]; a non-zero entry holds the channel;
 *                          NULL: nobody is held), holdoff (samples, 0 ... AFSK_MAX_STREAM_LEN, else AFSK_E_INVALID_ARG)
 *                          and out_deferred (DEVICE int64 [n_channels], not NULL).  hold is indexed by TRANSMITTER
 *                          channel and read when the kernels run, as d_lens_or_null is.  For channel c, with pos its
 *                          stream position before the pull, L the samples it advances (n_samples or clamp(lens[c], 0,
 *                          n_samples)), h = hold[c] != 0, and w the channel's wait counter (int32 state, 0 after create
 *                          and reset):
 *                            1. earliest = h ? pos + L : pos + w.
 *                            2. u = the oldest queued message with start >= pos: it has not begun.  A message with
 *                               start < pos is on air, or in its silent tail, and is never touched.
 *                            3. If u exists and u.start < earliest: delta = earliest - u.start; u and every message
 *                               behind it in the queue get start += delta, the channel's end (where the next submit
 *                               queues) gets += delta, out_deferred[c] = delta.  Otherwise out_deferred[c] = 0.
 *                            4. The pull renders and commits exactly as afsk_live_tx_pull_ragged would on the adjusted
 *                               queue: a message on air plays to its end, a held idle channel writes zeros, with w < L and
 *                               no hold a message begins w samples into the pull, out_pending counts as before.
 *                            5. w' = h ? holdoff : max(0, w - L).
 *                          So: messages queued back to back stay back to back; a later submit queues behind the shifted
 *                          end; every message is still exactly the samples of its payload at its rate, only later, by the
 *                          sum of the out_deferred values it lived through; a shift only widens the gap between two
 *                          messages.  With hold all zero (or NULL), holdoff 0 and w 0 the result is
 *                          afsk_live_tx_pull_ragged's bit for bit and out_deferred all 0.  A channel with L = 0 that is
 *                          held shifts nothing and sets w = holdoff.  afsk_live_tx_pull and afsk_live_tx_pull_ragged
 *                          neither read nor write w, and may alternate with hold pulls.  Works for transmitters of every
 *                          kind (one geometry, mixed, rated).  Two launches in order on hip_stream (one when n_samples
 *                          is 0), capturable into a graph.
 * Not part of this rule: random backoff (every released channel starts after exactly its wait) and muting a receiver
 * channel while its own transmitter is on air -- afsk_live_tx_pull_csma and afsk_live_push_muted below.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_TX_HOLD_SIGNATURES.)
 */
extern int afsk_live_busy(afsk_live *live, int32_t *d_out_busy, void *hip_stream);
extern int afsk_live_tx_pull_hold(afsk_live_tx *tx, int16_t *out, int64_t out_row_stride, int32_t n_samples,
                                  const int32_t *d_lens_or_null, const int32_t *d_hold_or_null, int32_t holdoff,
                                  int32_t *out_pending, int64_t *out_deferred, void *hip_stream);

/*
 * Half-duplex stations (added after ABI version 2; the version is unchanged): what carrier sense lacks to put a station
 * on a shared channel.  Two stations that heard the same burst are released by the same block and would key up on the
 * same sample, again on every retry: the csma pull spreads them with the KISS persistence rule.  A station whose own
 * output reaches its input would hold itself and, with afsk_live_tx_submit_events, repeat itself: the muted push does
 * not hear the columns it is told.  All of it is integer and sample-exact, and
 *   push_muted(mute = on_air) -> busy -> submit_events -> pull_csma(hold = busy)
 * stays one captured graph.
 *
 *  afsk_live_tx_pull_csma  afsk_live_tx_pull_hold (its arguments, its checks) with persist (0 ... 255, else
 *                          AFSK_E_INVALID_ARG), slot (samples, 0 ... 2^20, else AFSK_E_INVALID_ARG), seed (any uint32)
 *                          and out_on_air (DEVICE int32 [n_channels, 2], not NULL).  Steps 1-4 of the hold rule are
 *                          unchanged; with k the channel's draw counter (int32 state, 0 after create and reset) step 5
 *                          becomes
 *                            5. not held: w' = max(0, w - L), k' = k.
 *                               held:     with hash32(x) on uint32:  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 *                                         x *= 0x846ca68b; x ^= x >> 16 (the noise generator's hash),
 *                                           base = hash32(hash32(seed ^ hash32((uint32)c + 0x9e3779b9)) ^ (uint32)k),
 *                                           G = the smallest j in 0 ... 254 with (hash32(base ^ j) & 255) <= persist,
 *                                               255 when there is none,
 *                                         w' = holdoff + slot * G (below 2^31 by the bounds above), k' = k + 1 (uint32
 *                                         wrap-around).
 *                          So a released channel waits its holdoff plus a geometric number of slots, each taken with
 *                          probability (persist + 1) / 256: KISS p-persistence with the draws made at release; when the
 *                          carrier comes back, the next held pull draws again.  With persist = 255 G is 0: every sample,
 *                          out_pending and out_deferred are afsk_live_tx_pull_hold's bit for bit.  afsk_live_tx_pull,
 *                          _pull_ragged and _pull_hold neither read nor write k, and may alternate with this entry.
 *                          out_on_air[c] = (lo, hi): the hull, in columns of this pull, of the tone samples the pull
 *                          rendered for channel c -- over the channel's messages after step 3, each contributing
 *                          [start, start + n_samples - AFSK_TAIL_SILENCE) intersected with [pos, pos + L), relative to
 *                          pos; the silent tail is not on air; (0, 0) when there is no tone sample or L = 0.  Works for
 *                          transmitters of every kind.  Two launches in order on hip_stream (one when n_samples is 0):
 *                          the hold pull's tile kernel, which only reads w, and a commit kernel of its own.
 *  afsk_live_push_muted    afsk_live_push_ragged (its arguments, its checks, its outputs) with d_mute (DEVICE int32
 *                          [n_channels, 2], not NULL, read when the kernel runs) behind d_flush_mask_or_null.  Channel c
 *                          appends len_c samples as in the ragged push; with lo' = clamp(mute[c][0], 0, len_c) and hi' =
 *                          clamp(mute[c][1], lo', len_c), columns [lo', hi') of its row count as 0 wherever the push uses
 *                          them -- a block's amplitude, what is recorded or demodulated, and the partial block carried
 *                          to the next push (a muted sample that is carried is 0 in the next push too).  No column at
 *                          or beyond len_c is read.  Every output and the receiver's state equal, bit for bit, those of
 *                          afsk_live_push_ragged on a chunk whose columns [lo', hi') were zeroed.  For a receiver of any
 *                          kind but the auto-rate one; one launch (plus the stored receiver's demodulator launches), and
 *                          may alternate with the other pushes.  out_on_air of a pull of the same length is such an
 *                          array.
 *  afsk_live_push_auto_muted  the same for afsk_live_push_auto and a receiver of afsk_live_create_stream_auto (d_mute
 *                          again behind d_flush_mask_or_null).
 * Not part of the rule: persist / slot per channel; a draw for a message submitted to a channel that is clear and idle
 * (it starts at once); muting by anything but one column range per channel and push.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_CSMA_SIGNATURES.)
 */
extern int afsk_live_tx_pull_csma(afsk_live_tx *tx, int16_t *out, int64_t out_row_stride, int32_t n_samples,
                                  const int32_t *d_lens_or_null, const int32_t *d_hold_or_null, int32_t holdoff,
                                  int32_t persist, int32_t slot, uint32_t seed, int32_t *out_pending,
                                  int64_t *out_deferred, int32_t *out_on_air, void *hip_stream);
extern int afsk_live_push_muted(afsk_live *live, const int16_t *chunk, int64_t chunk_row_stride, int32_t chunk_len,
                                const int32_t *d_chunk_lens_or_null, int32_t flush, const uint8_t *d_flush_mask_or_null,
                                const int32_t *d_mute, int32_t *out_n_closed, int64_t *out_burst_start,
                                int32_t *out_burst_len, int32_t *out_flags, uint8_t *out_bytes, int32_t out_stride,
                                int32_t *out_nbytes, int32_t *out_nbits, int32_t *out_clock_idx, int32_t *out_term_frame,
                                int32_t *out_status, int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride,
                                uint8_t *tap_bytes, int32_t *tap_n, int32_t *tap_len, int64_t *open_start,
                                int32_t *open_nbytes, void *hip_stream);
extern int afsk_live_push_auto_muted(afsk_live *live, const int16_t *chunk, int64_t chunk_row_stride, int32_t chunk_len,
                                     const int32_t *d_chunk_lens_or_null, int32_t flush,
                                     const uint8_t *d_flush_mask_or_null, const int32_t *d_mute, int32_t *out_n_closed,
                                     int64_t *out_burst_start, int32_t *out_burst_len, int32_t *out_flags,
                                     uint8_t *out_bytes, int32_t out_stride, int32_t *out_nbytes, int32_t *out_nbits,
                                     int32_t *out_clock_idx, int32_t *out_term_frame, int32_t *out_status,
                                     int32_t *out_corrected, int32_t *out_margins, int32_t margin_stride,
                                     uint8_t *tap_bytes, int32_t *tap_n, int32_t *tap_len, int64_t *open_start,
                                     int32_t *open_nbytes, int32_t *out_bit_frames, int32_t *out_rate_score,
                                     void *hip_stream);

/*
 * The live medium (added after ABI version 2; the version is unchanged): the air between live stations.  Every output
 * row is the clipped sum of the source rows its links name, each scaled by a gain -- many stations per channel, hidden
 * terminals (a gain of 0 is no link), near / far levels, and receiver noise that continues from call to call.  The
 * reference has no counterpart (it opens one sound device).  All of it is integer and sample-exact.
 *
 *  afsk_live_mix        Sources are the rows of ONE int16 matrix src [n_src, >= n_samples] with src_row_stride samples
 *                       between rows -- a station's pull writes its rows in place, a capture or a background is more
 *                       rows.  Links are a CSR list per output row, all DEVICE int32 and read when the kernel runs:
 *                       d_row_ptr [n_out + 1], d_link_src [n_links], d_link_gain_q15 [n_links]; unity gain is 32768.
 *                       With T = n_samples, for output row r and column j in [0, T):
 *                         lo = clamp(row_ptr[r], 0, n_links)
 *                         hi = clamp(row_ptr[r + 1], lo, min(n_links, lo + 32768))
 *                         acc(r, j)  = sum over links k in [lo, hi) of term_k(j)
 *                         term_k(j)  = (g_k * x_k(j)) >> 15                  (arithmetic shift: floor)
 *                         g_k        = clamp(link_gain_q15[k], -65535, 65535)
 *                         x_k(j)     = src[link_src[k]][j]  if 0 <= link_src[k] < n_src and j < len_k,  else 0
 *                         len_k      = clamp(src_lens[link_src[k]], 0, T)    (T when d_src_lens_or_null is NULL)
 *                         out[r][j]  = clamp(acc(r, j), -32768, 32767)
 *                       Columns of a source at or beyond its length are NOT READ (a raggedly pulled buffer with stale
 *                       columns is safe), columns of out at or beyond T are not written, a row with no links is zeros.
 *                       A product fits int32 (65535 * 32768 < 2^31, both factors fit 24 bits) and so does a row's sum
 *                       (32768 * 65535 < 2^31).  With every gain 32768 the result equals, bit for bit,
 *                       clamp(sum of the int32 rows) -> int16.  A table that breaks the rules afsk_live_mix_check
 *                       enforces is clamped or ignored as written above: it cannot make the kernel read out of bounds.
 *                       Noise, when d_noise_scale_q24_or_null (DEVICE int32 [n_out]) is given: the result equals the
 *                       noiseless mix followed by afsk_add_noise_batch (its generator, its rounding, its second clip)
 *                       over the output rows taken as streams whose sample 0 is medium sample pos -- row r is stream
 *                       noise_idx_base + r (uint32) with seed noise_seed, column j has sample index (uint32)(pos + j),
 *                       a row whose scale is 0 draws nothing.  pos = *d_pos_or_null (DEVICE int64 [1], read when the
 *                       kernel runs; 0 when NULL).  When d_pos_or_null is given a second, one-thread launch behind the
 *                       mix adds n_samples to it, so a captured graph replays with continuing noise and two mixes of T
 *                       equal one mix of 2 T.
 *                       AFSK_E_INVALID_ARG: a NULL src / out / d_row_ptr / d_link_src / d_link_gain_q15 unless its
 *                       count (n_src / n_out / n_out / n_links / n_links) is 0; a negative count; n_samples outside
 *                       0 ... 2^20; a row stride below n_samples where there is more than one row; out's byte range
 *                       (first row's first column to last row's column T) overlapping src's; n_out * ceil(T / 2048)
 *                       above 2^31 - 1.  n_samples == 0 or n_out == 0 launches nothing and leaves pos unchanged.
 *                       Otherwise one launch, two with d_pos_or_null, in order on hip_stream, no host read: capturable.
 *  afsk_live_mix_check  host-only (no device needed), HOST arrays: AFSK_E_INVALID_ARG for a row_ptr that does not
 *                       start at 0, falls, or does not end at n_links; a row with more than 32768 links; a source
 *                       outside 0 ... n_src - 1; a gain outside -65535 ... 65535; a negative count or a NULL array
 *                       (the link arrays may be NULL when n_links is 0).
 * Not part of the rule: fading, more than one source matrix per call, a length per output row.  (A delay per link:
 * afsk_live_mix_delayed, a filter per link: afsk_live_mix_filtered, both below.)
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_MIX_SIGNATURES.)
 */
extern int afsk_live_mix(const int16_t *src, int64_t src_row_stride, int32_t n_src, const int32_t *d_src_lens_or_null,
                         const int32_t *d_row_ptr, const int32_t *d_link_src, const int32_t *d_link_gain_q15,
                         int32_t n_links, int16_t *out, int64_t out_row_stride, int32_t n_out, int32_t n_samples,
                         const int32_t *d_noise_scale_q24_or_null, uint32_t noise_seed, uint32_t noise_idx_base,
                         int64_t *d_pos_or_null, void *hip_stream);
extern int afsk_live_mix_check(const int32_t *h_row_ptr, const int32_t *h_link_src, const int32_t *h_link_gain_q15,
                               int32_t n_out, int32_t n_src, int32_t n_links);

/*
 * The delayed live medium (added after ABI version 2; the version is unchanged): afsk_live_mix with a delay in samples
 * per link -- the latency between stations that makes carrier sense imperfect (a station senses its neighbour only D
 * samples after it keyed up), and multipath (the same source on two links at two delays).  All of it is integer and
 * sample-exact.
 *
 * State, both on the DEVICE and owned by the caller:
 *   pos      int64 [1], as the noisy medium keeps it: the medium time the next mix begins at.
 *   history  int16 [n_src, hist_len], contiguous; hist_len a power of two in 8 ... 2^20.  The sample source s had at
 *            medium time t lies at history[s][t & (hist_len - 1)].  All zeros: nothing was sent yet.
 * X_s(t) is source row s as ONE signal over medium time: column j of the mix that began at position p is time p + j, a
 * column at or beyond that mix's clamp(src_lens[s], 0, T) is 0 (and is not read), and everything before the first mix,
 * or since the history was last zeroed, is 0.
 *
 *  afsk_live_mix_delayed   afsk_live_mix's arguments plus d_link_delay (DEVICE int32 [n_links], read when the kernel
 *                          runs), d_history and hist_len; d_pos is required.  With T = n_samples and pos = *d_pos read
 *                          when the kernel runs, for output row r and column j in [0, T):
 *                            d_k        = clamp(link_delay[k], 0, hist_len)
 *                            x_k(j)     = X_{link_src[k]}(pos + j - d_k)    (0 for a source outside 0 ... n_src - 1)
 *                            term_k(j)  = (g_k * x_k(j)) >> 15
 *                          and lo, hi, g_k, the clamp of the sum, out[r][j] and the noise on top exactly as
 *                          afsk_live_mix defines them.  x_k(j) comes from src when j - d_k >= 0 and from the history
 *                          otherwise.  Behind the mix, in order on hip_stream, a second launch writes
 *                            history[s][(pos + j) & (hist_len - 1)] = (j < len_s ? src[s][j] : 0)
 *                          for j in [max(0, T - hist_len), T) and every source row s (no launch when n_src is 0), and
 *                          a third, of one thread, adds T to pos.  The history is written only after the mix has read
 *                          it, so a delay equal to hist_len is legal: it reads the slot about to be overwritten.
 *                          With every delay 0 the output is afsk_live_mix's, bit for bit, noise included; two mixes
 *                          of T equal one of 2 T; T may be smaller than, equal to or larger than hist_len.  A delay
 *                          or a source out of range in the device table is clamped or ignored as written above before
 *                          anything is read through it.
 *                          AFSK_E_INVALID_ARG: everything afsk_live_mix refuses; a hist_len that is not a power of two
 *                          in 8 ... 2^20; a NULL d_pos; a NULL d_history when n_src > 0; a NULL d_link_delay when
 *                          n_links > 0; a history whose bytes [d_history, + 2 * n_src * hist_len) overlap src's or
 *                          out's byte range; n_out * ceil(T / 2048) or n_src * ceil(min(T, hist_len) / 2048) above
 *                          2^31 - 1.  n_samples == 0 or n_out == 0 launches nothing and leaves pos and the history
 *                          as they were.  Otherwise three launches (live_mix_delay_kernel, live_mix_history_kernel,
 *                          live_mix_advance_kernel), no allocation, no host read: capturable.
 *  afsk_live_mix_delayed_check  host-only (no device needed), HOST arrays: afsk_live_mix_check's rules, and
 *                          AFSK_E_INVALID_ARG for a hist_len as above, a NULL h_link_delay when n_links > 0 or a delay
 *                          outside 0 ... hist_len.
 * Not part of the rule: fractional-sample delays, delays that change while the medium runs (the table is the caller's,
 * but the history holds no more than hist_len samples; a filter per link: afsk_live_mix_filtered, fading:
 * afsk_live_mix_faded, both below), clearing the history of single rows, a length per output row, more than one source
 * matrix per call.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_DELAY_SIGNATURES.)
 */
extern int afsk_live_mix_delayed(const int16_t *src, int64_t src_row_stride, int32_t n_src,
                                 const int32_t *d_src_lens_or_null, const int32_t *d_row_ptr, const int32_t *d_link_src,
                                 const int32_t *d_link_gain_q15, const int32_t *d_link_delay, int32_t n_links,
                                 int16_t *out, int64_t out_row_stride, int32_t n_out, int32_t n_samples,
                                 const int32_t *d_noise_scale_q24_or_null, uint32_t noise_seed, uint32_t noise_idx_base,
                                 int64_t *d_pos, int16_t *d_history, int32_t hist_len, void *hip_stream);
extern int afsk_live_mix_delayed_check(const int32_t *h_row_ptr, const int32_t *h_link_src,
                                       const int32_t *h_link_gain_q15, const int32_t *h_link_delay, int32_t n_out,
                                       int32_t n_src, int32_t n_links, int32_t hist_len);

/*
 * The filtered live medium (added after ABI version 2; the version is unchanged): afsk_live_mix_delayed with an FIR
 * filter in Q14 taps per link -- the band limit of a radio audio path, a telephone line or a speaker into a microphone,
 * multipath on one link as several taps, pre- and de-emphasis.  All of it is integer and sample-exact.
 *
 * The filter table, on the DEVICE and owned by the caller, is n_filters filters stored as CSR:
 *   filter_ptr   int32 [n_filters + 1]: filter f has K_f = filter_ptr[f + 1] - filter_ptr[f] taps, 1 <= K_f <= 256.
 *   filter_taps  int16 [n_taps], Q14: unity is 16384, a tap lies in -32768 ... 32767; for every filter the sum of |h|
 *                is at most 65535 (an L1 gain below 4), so that sum |h| * 32768 < 2^31.
 *   link_filter  int32 [n_links]: the link's filter, -1 for none.
 * pos, the history and X_s(t) are afsk_live_mix_delayed's, unchanged.
 *
 *  afsk_live_mix_filtered   afsk_live_mix_delayed's arguments plus d_link_filter (behind d_link_delay) and
 *                          d_filter_ptr, d_filter_taps, n_filters and n_taps (behind hist_len).  For a link k with
 *                          filter f = link_filter[k] >= 0, taps h = filter_taps + filter_ptr[f] and K = K_f:
 *                            d_k        = clamp(link_delay[k], 0, hist_len - (K - 1))
 *                            v_k(j)     = sum_{i = 0 .. K - 1} h[i] * X_{link_src[k]}(pos + j - d_k - i)     (int32, exact)
 *                            f_k(j)     = clamp(v_k(j) >> 14, -32768, 32767)          (arithmetic shift: floor)
 *                            term_k(j)  = (g_k * f_k(j)) >> 15
 *                          A link with link_filter[k] == -1 contributes afsk_live_mix_delayed's term, bit for bit.
 *                          The row sum, the clip, the noise, the position and the history ring are that entry's.  The
 *                          reach of a filtered link is d + K - 1 and must not exceed hist_len.  So the identity filter
 *                          {16384} on every link gives afsk_live_mix_delayed's output bit for bit, noise included; n
 *                          zero taps in front of {16384} on a link at delay d equal that link unfiltered at delay
 *                          d + n; and two mixes of T equal one of 2 T, for any T against hist_len and against K.
 *                          Device clamps, applied before anything is read through an entry: afsk_live_mix_delayed's;
 *                          a link_filter below -1 or >= n_filters makes the link silent; filter_ptr entries are clamped
 *                          into [0, n_taps] and the second not below the first; K to 0 ... min(256, hist_len + 1), and
 *                          K = 0 is silent; the delay as written above.  Taps are values, not addresses: a table whose
 *                          sum of |h| exceeds 65535 (afsk_live_mix_filtered_check refuses it) may wrap v_k in 32 bits
 *                          -- that result is not defined here -- and is memory-safe all the same.
 *                          AFSK_E_INVALID_ARG: everything afsk_live_mix_delayed refuses; a negative n_filters or
 *                          n_taps; a NULL d_filter_ptr; a NULL d_filter_taps when n_taps > 0; a NULL d_link_filter
 *                          when n_links > 0.  n_samples == 0 or n_out == 0 launches nothing.  Otherwise three launches
 *                          (live_mix_fir_kernel, live_mix_history_kernel, live_mix_advance_kernel), no allocation, no
 *                          host read: capturable.
 *  afsk_live_mix_filtered_check  host-only (no device needed), HOST arrays: afsk_live_mix_delayed_check's rules, and
 *                          AFSK_E_INVALID_ARG, naming the filter or the link, for a filter_ptr that does not start at
 *                          0, or does not rise to n_taps; a filter with K outside 1 ... 256 or a sum of |h| above
 *                          65535; a link_filter outside -1 ... n_filters - 1; a filtered link whose reach exceeds
 *                          hist_len; a NULL array (h_filter_taps may be NULL when n_taps is 0).
 * Not part of the rule: taps that change while the medium runs (a gain that does: afsk_live_mix_faded, below), IIR
 * sections, fractional-sample delays, a filter per output row, filters longer than 256 taps.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_FIR_SIGNATURES.)
 */
extern int afsk_live_mix_filtered(const int16_t *src, int64_t src_row_stride, int32_t n_src,
                                  const int32_t *d_src_lens_or_null, const int32_t *d_row_ptr, const int32_t *d_link_src,
                                  const int32_t *d_link_gain_q15, const int32_t *d_link_delay,
                                  const int32_t *d_link_filter, int32_t n_links, int16_t *out, int64_t out_row_stride,
                                  int32_t n_out, int32_t n_samples, const int32_t *d_noise_scale_q24_or_null,
                                  uint32_t noise_seed, uint32_t noise_idx_base, int64_t *d_pos, int16_t *d_history,
                                  int32_t hist_len, const int32_t *d_filter_ptr, const int16_t *d_filter_taps,
                                  int32_t n_filters, int32_t n_taps, void *hip_stream);
extern int afsk_live_mix_filtered_check(const int32_t *h_row_ptr, const int32_t *h_link_src,
                                        const int32_t *h_link_gain_q15, const int32_t *h_link_delay,
                                        const int32_t *h_link_filter, int32_t n_out, int32_t n_src, int32_t n_links,
                                        int32_t hist_len, const int32_t *h_filter_ptr, const int16_t *h_filter_taps,
                                        int32_t n_filters, int32_t n_taps);

/*
 * The faded live medium (added after ABI version 2; the version is unchanged): afsk_live_mix_filtered with a gain per
 * link that moves along a cyclic Q15 track while the medium runs -- a signal that sinks under a receiver's gate for
 * half a second, a station in reach on one tick and hidden on the next, the two delayed copies of a two-ray HF channel
 * fading independently.  All of it is integer and sample-exact, and the envelope is a pure function of the position and
 * the tables: a faded medium has no state beyond the delayed medium's.
 *
 * The fade table, on the DEVICE and owned by the caller, is n_fades tracks stored as CSR:
 *   fade_ptr     int32 [n_fades + 1]: track f has L_f = fade_ptr[f + 1] - fade_ptr[f] knots, a power of two in
 *                1 ... 65536.
 *   fade_shift   int32 [n_fades]: p_f in 3 ... 15; the track has 2^p_f samples per knot (8 ... 32768) and is cyclic
 *                with period L_f * 2^p_f samples, which divides 2^32.
 *   fade_knots   uint16 [n_knots], Q15 gains: 32768 is unity, 0 no signal, 65535 just under x 2.
 *   link_fade    int32 [n_links]: the link's track, -1 for none.
 *   link_fade_offset  uint32 [n_links]: where in its track the link is at medium time 0, in samples (any value).
 * pos, the history, X_s(t), d_k, v_k and f_k are afsk_live_mix_filtered's, unchanged.
 *
 *  afsk_live_mix_faded     afsk_live_mix_filtered's arguments plus d_link_fade, d_link_fade_offset, d_fade_ptr,
 *                          d_fade_shift, d_fade_knots, n_fades and n_knots (behind n_taps).  For a link k with track
 *                          f = link_fade[k] >= 0, knots = fade_knots + fade_ptr[f], L = L_f and p = p_f, at column j
 *                          (medium time pos + j, the LISTENER's time: not pos + j - d_k):
 *                            u        = (uint32)(pos + j) + link_fade_offset[k]                    (mod 2^32)
 *                            n        = (u >> p) & (L - 1);   m = (n + 1) & (L - 1);   q = u & (2^p - 1)
 *                            e_k(j)   = knots[n] + (((int32)(knots[m] - knots[n]) * q) >> p)
 *                                       (arithmetic shift: floor; |product| < 65536 * 2^15 = 2^31)
 *                            x_k(j)   = X_{link_src[k]}(pos + j - d_k) without a filter, f_k(j) with one
 *                            term_k(j) = (g_k * clamp((e_k(j) * x_k(j)) >> 15, -32768, 32767)) >> 15
 *                          e_k lies between its two knots, so in 0 ... 65535, and e_k * x_k fits int32
 *                          (65535 * 32768 < 2^31).  With e_k = 32768 the term is the filtered medium's exactly, so a
 *                          unity track on every link gives afsk_live_mix_filtered's output bit for bit, noise included.
 *                          A link with link_fade[k] == -1 contributes afsk_live_mix_filtered's term, bit for bit.  The
 *                          row sum, the clip, the noise, the position and the history ring are that entry's.  Since
 *                          L * 2^p divides 2^32 the envelope depends on the low 32 bits of pos alone and is continuous
 *                          past 2^32 samples; since it depends on nothing but pos and the tables, two mixes of T
 *                          equal one of 2 T, afsk_live_mix_delayed's state is the whole state, and a captured graph
 *                          replays.  fade_knots is read when the kernels run: the caller may rewrite it between
 *                          calls (a scripted event, a track updated live), in stream order.
 *                          Device clamps, applied before anything is read through an entry: afsk_live_mix_filtered's;
 *                          a link_fade below -1 or >= n_fades makes the link silent; fade_ptr entries are clamped into
 *                          [0, n_knots] and the second not below the first; L is their difference rounded down to a
 *                          power of two, at most 65536, and no knots make the link silent; the shift is clamped to
 *                          3 ... 15.  Knots and offsets are values, not addresses.
 *                          AFSK_E_INVALID_ARG: everything afsk_live_mix_filtered refuses; a negative n_fades or
 *                          n_knots; a NULL d_fade_ptr; a NULL d_fade_shift when n_fades > 0; a NULL d_fade_knots when
 *                          n_knots > 0; a NULL d_link_fade or d_link_fade_offset when n_links > 0.  n_samples == 0 or
 *                          n_out == 0 launches nothing.  Otherwise three launches (live_mix_fade_kernel,
 *                          live_mix_history_kernel, live_mix_advance_kernel), no allocation, no host read: capturable.
 *  afsk_live_mix_faded_check  host-only (no device needed), HOST arrays: afsk_live_mix_filtered_check's rules
 *                          (n_filters = 0 with filter_ptr = {0} is legal), and AFSK_E_INVALID_ARG, naming the track or
 *                          the link, for a fade_ptr that does not start at 0, or does not rise to n_knots; a track
 *                          whose L is not a power of two in 1 ... 65536 or whose shift is outside 3 ... 15; a
 *                          link_fade outside -1 ... n_fades - 1; a NULL array (h_fade_shift may be NULL when n_fades
 *                          is 0).  The knots and the offsets need no check: every value is legal.
 * Not part of the rule: phase or complex fading, tracks whose length or period is no power of two, a track per output
 * row, generating tracks on the device.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_FADE_SIGNATURES.)
 */
extern int afsk_live_mix_faded(const int16_t *src, int64_t src_row_stride, int32_t n_src,
                               const int32_t *d_src_lens_or_null, const int32_t *d_row_ptr, const int32_t *d_link_src,
                               const int32_t *d_link_gain_q15, const int32_t *d_link_delay,
                               const int32_t *d_link_filter, int32_t n_links, int16_t *out, int64_t out_row_stride,
                               int32_t n_out, int32_t n_samples, const int32_t *d_noise_scale_q24_or_null,
                               uint32_t noise_seed, uint32_t noise_idx_base, int64_t *d_pos, int16_t *d_history,
                               int32_t hist_len, const int32_t *d_filter_ptr, const int16_t *d_filter_taps,
                               int32_t n_filters, int32_t n_taps, const int32_t *d_link_fade,
                               const uint32_t *d_link_fade_offset, const int32_t *d_fade_ptr,
                               const int32_t *d_fade_shift, const uint16_t *d_fade_knots, int32_t n_fades,
                               int32_t n_knots, void *hip_stream);
extern int afsk_live_mix_faded_check(const int32_t *h_row_ptr, const int32_t *h_link_src,
                                     const int32_t *h_link_gain_q15, const int32_t *h_link_delay,
                                     const int32_t *h_link_filter, const int32_t *h_link_fade, int32_t n_out,
                                     int32_t n_src, int32_t n_links, int32_t hist_len, const int32_t *h_filter_ptr,
                                     const int16_t *h_filter_taps, int32_t n_filters, int32_t n_taps,
                                     const int32_t *h_fade_ptr, const int32_t *h_fade_shift, int32_t n_fades,
                                     int32_t n_knots);

/*
 * The duplicate filter (added after ABI version 2; the version is unchanged): the list every digipeater keeps so that
 * two relays that hear each other do not repeat each other for ever -- a payload already handled within the last
 * `window` samples is not repeated.  The reference protocol has no framing, no addresses and no hop count, so payload
 * identity within a time window is the only loop breaker it can have.  afsk_live_push_muted breaks the loop of a station
 * with itself; this breaks the loop between stations.  All of it is integer and exact, and
 *   push_muted -> busy -> dedup_filter -> submit_events_kept -> pull_csma -> mix
 * stays one captured graph.
 *
 * State.  Every receiver channel owns a ring of `depth` entries (1 ... 64), an entry {uint64 key; int64 time}, time
 * INT64_MIN: the entry is empty; and an int32 head, the entry the next insertion writes.  One DEVICE allocation:
 *   [0, 16 * n_channels * depth)      the entries, channel-major
 *   [o_head, + 4 * n_channels)        the heads; o_head = the entries' bytes rounded up to 256
 *   [o_scratch, + 256)                scratch of the order kernels; o_scratch = o_head + (4 * n_channels rounded up to 256)
 * 65536 channels at depth 8 hold 8 MiB of entries.
 *
 * The key of a payload p[0 .. n), all arithmetic mod 2^64:
 *   mix64(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *              z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   key = mix64( (sum over i < n of mix64(((uint64)i << 8) | p[i])) ^ ((uint64)n << 32) )
 * (the sum commutes: a wave adds its lanes' terms in any order and still gets the exact value).
 *
 * The rule, for the eligible items of ONE channel in list order, each with its key and a time t:
 *   duplicate  some non-empty entry of the channel has the same key, entry.time <= t and t - entry.time < window (the
 *              age is taken without overflow): AFSK_LIVE_DEDUP_DUP.  The table stays as it is; the entry's time is NOT
 *              refreshed.
 *   new        otherwise: {key, t} is written at ring[head], head becomes (head + 1) % depth: AFSK_LIVE_DEDUP_NEW.  This
 *              replaces the oldest insertion whether or not it has expired.
 * A later item of the same list sees the insertion an earlier one made: two equal bursts in one list are NEW, then DUP.
 * window (int64 samples, >= 0) comes with every call; window 0 remembers everything and drops nothing.  An entry from
 * the future (t < entry.time: the stream restarted after a reset or a flush) is no duplicate.  (A time of exactly
 * INT64_MIN is stored as it is and reads as an empty entry.)
 * A burst is remembered when it is HEARD, not when it is queued: a burst the transmitter then refuses
 * (AFSK_LIVE_TX_QUEUE_FULL, _TOO_LONG ...) is on the list all the same, and a second copy of it within the window is a
 * duplicate.
 *
 *  afsk_live_dedup_layout   host-only (no device needed): the state's bytes as above.  AFSK_E_INVALID_ARG: n_channels
 *                           < 1, depth outside 1 ... 64.
 *  afsk_live_dedup_create   allocates the state on the current device, every ring empty, every head 0 (synchronous).
 *  afsk_live_dedup_destroy  after the launches that use the filter have completed (NULL is fine).
 *  afsk_live_dedup_reset    empties the rings of every channel (d_mask_or_null NULL) or of the channels whose DEVICE
 *                           uint8 mask entry is non-zero and sets their heads to 0; one launch on hip_stream.
 *  afsk_live_dedup_get_state / _set_state  synchronous copies of the entries and the heads -- bytes [0, o_scratch) of
 *                           the state, `bytes` must be exactly that -- to and from HOST memory: a station that restarts
 *                           keeps its list.  _set_state refuses a head outside 0 ... depth - 1.
 *  afsk_live_dedup_filter   filters the packed event list of one push.  The records are read exactly as
 *                           afsk_live_tx_submit_events reads them: `stored` is clamped to 0 ... max_events and the first
 *                           unsorted record is found by the same order kernel, writing into the filter's own scratch.
 *                           d_verdict (DEVICE int32 [max_events], all written by every call), entry i:
 *                             i >= stored                                   AFSK_LIVE_DEDUP_NONE
 *                             at or past the first unsorted record, or the
 *                             record is not eligible                        AFSK_LIVE_DEDUP_PASS: neither looked up nor
 *                                                                           remembered; whatever consumes the list
 *                                                                           decides (the relay answers _UNSORTED,
 *                                                                           _SKIPPED ... as it does without a filter)
 *                             otherwise                                     the rule with t = burst_start + burst_len
 *                           A record is eligible when its channel lies in 0 ... n_channels - 1, its status is
 *                           AFSK_ST_OK, 1 <= nbytes <= out_stride, payload_offset >= 0, payload_offset + nbytes <=
 *                           max_bytes and flags & (skip_flags | AFSK_LIVE_OVERFLOW) is 0: the relay's relayable
 *                           condition without the channel map.  Two launches in order on hip_stream (the order kernel,
 *                           live_dedup_kernel), no allocation, no synchronisation, no host read: capturable.  Nothing of
 *                           the events buffer is written, and whatever it holds no access leaves the buffers given.
 *  afsk_live_dedup_note     the same rule on explicit messages, so that an originating station puts what it sends on its
 *                           own list: d_channels int32 [n_messages], ascending (a message at or past the first one whose
 *                           channel is below its predecessor's gets _PASS); d_payload uint8 [n_messages,
 *                           payload_stride], row i the bytes of message i; d_payload_len int32 [n_messages]; d_time
 *                           int64 [n_messages], the message's t -- typically the submit's start + n_samples, the sample
 *                           at which a listener's burst of it ends.  A message whose length lies outside 1 ...
 *                           payload_stride or whose channel lies outside the filter's gets _PASS.  All DEVICE arrays.
 *                           Two launches (afsk_live_tx_submit's order kernel, live_dedup_note_kernel), capturable.
 *  afsk_live_tx_submit_events_kept  afsk_live_tx_submit_events_rated's arguments with d_rx_bit_frames_or_null nullable
 *                           (NULL: afsk_live_tx_submit_events' behaviour, on a rated transmitter table entry 0) and
 *                           d_keep (DEVICE int32 [max_events]) behind rx_slots.  A relayable record whose d_keep entry is
 *                           0 answers AFSK_LIVE_TX_DUPLICATE, start -1, n_samples 0, and takes no queue slot: the check
 *                           comes behind the _SKIPPED conditions and in front of _BAD_CHANNEL.  Any other d_keep value:
 *                           exactly what afsk_live_tx_submit_events / _rated do.  d_keep is read for relayable records
 *                           alone.  Uniform, mixed and rated transmitters; two launches, capturable.  Besides
 *                           afsk_live_tx_submit_events' refusals: a NULL d_keep; d_rx_bit_frames with rx_slots < 1 or
 *                           with a transmitter that is not rated.
 * AFSK_E_INVALID_ARG, nothing launched: a NULL filter, events, verdict or message array; a negative size or window;
 * skip_flags with bits other than AFSK_LIVE_OPEN_END | AFSK_LIVE_OVERFLOW; an events pointer that is not 16-byte aligned.
 * max_events == 0 or n_messages == 0: AFSK_OK, no launch.  Calls on one filter must run in order.
 * Not part of the rule: a window per channel, keys that ignore part of the payload, one list shared across channels,
 * refreshing an entry on a duplicate, a compacted copy of the event list.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_DEDUP_SIGNATURES.)
 */
#define AFSK_LIVE_DEDUP_NONE (-1) /* the entry is at or past `stored`: no record                                      */
#define AFSK_LIVE_DEDUP_DUP 0     /* handled within the window: do not repeat it                                       */
#define AFSK_LIVE_DEDUP_NEW 1     /* not on the list: remembered now                                                   */
#define AFSK_LIVE_DEDUP_PASS 2    /* not eligible or unsorted: not looked up, not remembered                           */
#define AFSK_LIVE_TX_DUPLICATE 7  /* afsk_live_tx_submit_events_kept: d_keep says 0 for this record: nothing queued    */
typedef struct afsk_live_dedup afsk_live_dedup;
extern int afsk_live_dedup_layout(int32_t n_channels, int32_t depth, int64_t *out_state_bytes);
extern int afsk_live_dedup_create(int32_t n_channels, int32_t depth, afsk_live_dedup **out);
extern int afsk_live_dedup_destroy(afsk_live_dedup *dd);
extern int afsk_live_dedup_reset(afsk_live_dedup *dd, const uint8_t *d_mask_or_null, void *hip_stream);
extern int afsk_live_dedup_get_state(afsk_live_dedup *dd, void *host_out, int64_t bytes);
extern int afsk_live_dedup_set_state(afsk_live_dedup *dd, const void *host_in, int64_t bytes);
extern int afsk_live_dedup_filter(afsk_live_dedup *dd, const void *events, int32_t max_events, int32_t max_bytes,
                                  int32_t out_stride, int32_t skip_flags, int64_t window, int32_t *d_verdict,
                                  void *hip_stream);
extern int afsk_live_dedup_note(afsk_live_dedup *dd, const int32_t *d_channels, const uint8_t *d_payload,
                                int32_t payload_stride, const int32_t *d_payload_len, const int64_t *d_time,
                                int32_t n_messages, int64_t window, int32_t *d_verdict, void *hip_stream);
extern int afsk_live_tx_submit_events_kept(afsk_live_tx *tx, const void *events, int32_t max_events, int32_t max_bytes,
                                           int32_t out_stride, int32_t n_rx_channels,
                                           const int32_t *d_channel_map_or_null, int32_t skip_flags,
                                           const int32_t *d_rx_bit_frames_or_null, int32_t rx_slots,
                                           const int32_t *d_keep, int32_t *out_status, int64_t *out_start,
                                           int32_t *out_n_samples, void *hip_stream);

/*
 * The level tracker of the streaming live receivers: a noise floor F and a decaying peak P per channel, followed on the
 * device block by block, and the channel's gate / squelch pair set from them ahead of every push -- so a channel at any
 * level opens its gate without the caller knowing that level.  Integer and exact:
 *   blocks   for channel c the whole 2048-sample blocks the push of the same arguments will walk: cl = pos & 2047 carried
 *            samples, len = chunk_len or clamp(d_chunk_lens[c], 0, chunk_len), nblk = (cl + len) / 2048, block 0 of a push
 *            with a carry = carry[0, cl) + chunk[0, 2048 - cl).  Nothing at or beyond column len is read.  A block's
 *            amplitude A is the gate's: sum |x| >> 11.  A block with any column inside the channel's clamped mute range
 *            (afsk_live_push_muted's clamp of d_mute[c]) is skipped: it is not loaded and updates nothing.
 *   update   rec = (the channel's gate is recording when the push starts), pp = P; for every block that is not skipped
 *              P  = A > P ? A : P - ((P - A + (1 << decay_shift) - 1) >> decay_shift)
 *              pp = max(pp, P)
 *              if (!rec)  F = F < 0 ? A : (A < F ? F - ((F - A + 3) >> 2) : F + ((A - F) >> rise_shift))
 *   pair     F and P are stored; unless rec, with Fz = max(F, 0)
 *              start = min(65535, max((start_q15 * pp) >> 15, (floor_start_q8 * Fz) >> 8, min_start))
 *              end   = min(65535, max((end_q15   * pp) >> 15, (floor_end_q8   * Fz) >> 8, min_end))
 *            go to the receiver's own pair of channel c and to the channel's state row.  While a burst records the pair
 *            stays what it was when the burst opened.
 *  afsk_live_create_stream_leveled  the streaming receiver of afsk_live_create_stream_thresholds (tap = 0) /
 *                           afsk_live_create_stream_tap (tap = 1) with bit_frames_host_or_null [n_channels] and n_cand = 0
 *                           (cand_bit_frames_host is then not read), or of afsk_live_create_stream_auto with n_cand > 0
 *                           (bit_frames_host_or_null is then not read), with those entries' checks -- kept in the
 *                           per-channel threshold layout even when all pairs agree, so that afsk_live_level can rewrite
 *                           the pairs.  It is pushed with the entries its kind is pushed with.
 *  afsk_live_level_check    host-only: AFSK_OK when 0 <= end_q15 <= start_q15 <= 65535, 0 <= floor_end_q8 <=
 *                           floor_start_q8 <= 65535, 0 <= min_end <= min_start <= 65535 and both shifts lie in 0 ... 15.
 *  afsk_live_level          d_state: DEVICE int32 [n_channels, 4], a row = (floor, peak, start, end), the caller's (rows
 *                           start as (-1, 0, amp_start, amp_end): afsk_live_level_reset).  chunk, chunk_row_stride,
 *                           chunk_len, d_chunk_lens_or_null, d_mute_or_null: what the push behind it is given.  ONE launch
 *                           (live_level_kernel, a wave per channel), asynchronous on hip_stream, no allocation, no host
 *                           read: capturable, and a graph of tracker + push is a linear chain.  chunk_len == 0: AFSK_OK,
 *                           no launch.  AFSK_E_INVALID_ARG, nothing launched: a stored receiver, a receiver of another
 *                           create entry, a NULL live, d_state or (chunk_len > 0) chunk, a negative size, chunk_len above
 *                           the receiver's max_chunk_len, params that afsk_live_level_check refuses.
 *  afsk_live_level_reset    rows of the channels where d_mask_or_null is non-zero (NULL: all) go back to (-1, 0,
 *                           amp_start0, amp_end0), and so do those channels' entries of the receiver's pair.  One launch.
 * Not part of the rule: the stored receiver, thresholds that move inside a burst, parameters per channel, scaling the
 * samples.
 * (Declared `extern int`: afskmodem_amd/_native.py binds them from a table of their own, LIVE_LEVEL_SIGNATURES.)
 */
typedef struct afsk_live_level_params {
    int32_t start_q15, end_q15;             /* the pair as Q15 ratios of the peak (18000 / 14000: the reference's) */
    int32_t floor_start_q8, floor_end_q8;   /* ... and as Q8 multiples of the noise floor (512 / 384)              */
    int32_t min_start, min_end;             /* ... and their least values (1024 / 768)                             */
    int32_t decay_shift, rise_shift;        /* the peak's decay and the floor's rise per block (2 / 6)             */
} afsk_live_level_params;
extern int afsk_live_create_stream_leveled(int32_t n_channels, const int32_t *bit_frames_host_or_null,
                                           const int32_t *cand_bit_frames_host, int32_t n_cand, int32_t max_score,
                                           const int32_t *amp_start_host, const int32_t *amp_end_host,
                                           int32_t max_payload_len, int32_t max_chunk_len, int32_t tap, afsk_live **out);
extern int afsk_live_level_check(afsk_live_level_params params);
extern int afsk_live_level(afsk_live *live, int32_t *d_state, afsk_live_level_params params, const int16_t *chunk,
                           int64_t chunk_row_stride, int32_t chunk_len, const int32_t *d_chunk_lens_or_null,
                           const int32_t *d_mute_or_null, void *hip_stream);
extern int afsk_live_level_reset(afsk_live *live, int32_t *d_state, const uint8_t *d_mask_or_null, int32_t amp_start0,
                                 int32_t amp_end0, void *hip_stream);

/*
 * Deterministic additive noise (build-owned test/benchmark input generator, no
 * reference counterpart): per sample an Irwin-Hall sum of 16 uniform u16 drawn
 * from a counter hash of (seed, stream_idx_base + s, sample index), centred,
 * multiplied by scale_q24[s] / 2^24, added and clipped to int16.  Integer-only,
 * so the CPU oracle's generator produces identical samples.
 */
int afsk_add_noise_batch(int16_t *samples, const int64_t *stream_offset,
                         const int32_t *stream_len, int32_t max_stream_len,
                         const int32_t *scale_q24, int32_t n_streams, uint32_t seed,
                         uint32_t stream_idx_base, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
