// fin_kernels.h -- host-callable launchers of the HIP kernels (implemented in fin_kernels.hip)
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fin_format.h"

#define FIN_FAST_CHUNKS 8   // the fast pre-pass keeps a read's chunks of one strand in LDS: reads of up to 256 bases (and the fused ingest needs no longer ones)

#ifdef __cplusplus
extern "C" {
#endif
int fin_launch_search_v0(const FinDevIndex* ix, const uint8_t* bases, const uint64_t* offs, const uint64_t* out_offs,
                         void* out, uint32_t n_reads, int strands, uint32_t lds_deque_limit, uint32_t* ovf_list, uint32_t* ovf_count,
                         uint64_t* ovf_scratch, uint32_t ovf_blocks, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);
int fin_launch_overflow(const FinDevIndex* ix, const uint8_t* bases, const uint64_t* offs, const uint64_t* out_offs, void* out,
                        int strands, const uint32_t* ovf_list, const uint32_t* ovf_count, uint64_t* ovf_scratch, uint32_t ovf_blocks,
                        hipStream_t stream);
int fin_launch_pack_reads(const uint8_t* bases, const uint64_t* offs, const FinReadDesc* desc, void* packed, uint32_t n_reads, uint64_t n_chunks, hipStream_t stream);
int fin_launch_search_v2(const FinDevIndex* ix, const uint8_t* bases, const void* packed, const FinReadDesc* desc,
                         const uint64_t* offs, const uint64_t* out_offs, void* out, uint64_t n_kmers, uint32_t n_reads,
                         int strands, uint32_t lds_deque_limit, uint32_t* ovf_list, uint32_t* ovf_count,
                         uint32_t* work_counter, uint64_t* ovf_scratch, uint32_t ovf_blocks, uint32_t grid_blocks,
                         hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);
int fin_v2_blocks_per_cu(void);
// v3 = v2 + walk mode, cold restart and probing (fin_kernel_v3.hip); same arguments
int fin_launch_search_v3(const FinDevIndex* ix, const uint8_t* bases, const void* packed, const FinReadDesc* desc,
                         const uint64_t* offs, const uint64_t* out_offs, void* out, uint64_t n_kmers, uint32_t n_reads,
                         int strands, uint32_t lds_deque_limit, uint32_t* ovf_list, uint32_t* ovf_count,
                         uint32_t* work_counter, uint64_t* ovf_scratch, uint32_t ovf_blocks, uint32_t grid_blocks,
                         uint32_t* pass /* 2 * n_reads + 4 words for the probe pre-pass, or NULL: probe inside the search kernel */,
                         uint32_t grid_blocks_probe, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev_mid /* between pre-pass and search */);
int fin_v3_blocks_per_cu(void);
// single-stage launchers used by kernel 4's pipeline (fin_kernel_w.hip)
int fin_launch_probe_stage(const FinDevIndex* ix, const void* packed, const FinReadDesc* desc, uint32_t n_reads, int strands, uint32_t* pass,
                           uint32_t* seed /* 2 * n_reads + 4 words: the seed node of every verdict, or NULL */, uint32_t* work_counter, uint32_t grid_blocks,
                           void* fast_out /* the batch's pairs when the fast path may write them (nothing prefills the output), else NULL */, uint32_t* n_fast,
                           const uint8_t* bases, const uint64_t* offs /* fused ingest (fin_launch_pair_prepass), else NULL */, hipStream_t stream);
int fin_launch_stream_stage(const FinDevIndex* ix, const void* packed, const FinReadDesc* desc, uint32_t lds_deque_limit, uint32_t* ovf_list,
                            uint32_t* ovf_count, uint32_t* work_counter, const void* items_in, const uint32_t* n_in, void* items_out,
                            uint32_t* n_out, uint32_t grid_blocks, hipStream_t stream);
int fin_launch_v3_list(const FinDevIndex* ix, const void* packed, const FinReadDesc* desc, void* out, int strands, uint32_t lds_deque_limit,
                       uint32_t* ovf_list, uint32_t* ovf_count, uint32_t* work_counter, const uint32_t* pass, const uint32_t* read_list,
                       const uint32_t* n_list, uint32_t grid_blocks, hipStream_t stream);
// the pair pre-pass (fin_prepass.hip): verdicts and seeds of both strands of every read; defer: one of them FIN_PASS_DEFERRED where possible
// out (may be NULL): the batch's pairs -- with it, a read the FAST PATH finishes (whole read against one unitig's text, gaps proven absent by
// the canonical string filter) is written here and gets the verdict FIN_PASS_DONE on both strands; n_fast (may be NULL): how many
// bases, offs (may be NULL): FUSED INGEST -- the fast kernels pack the ASCII reads themselves and write the chunks of every read they do not finish
// (a read they finish has undefined chunks); only where fin_pair_prepass_fuses() and no read is longer than ix->pp_max_len <= FIN_FAST_CHUNKS * 32
// bases, else an error.  Then n_fast (if not NULL) has three words: [1] += reads parked in LDS for phases 2 and 3 (ix->pp_park, ix->pp_park_cap),
// [2] += reads of list A beyond a block's park area
int fin_launch_pair_prepass(const FinDevIndex* ix, const void* packed, const FinReadDesc* desc, uint32_t n_reads, uint32_t* pass, uint32_t* seed,
                            int defer, uint32_t grid_hint, void* out, uint32_t* n_fast, const uint8_t* bases, const uint64_t* offs, hipStream_t stream);
// 1: fin_launch_pair_prepass with out and defer runs a fast kernel on this index, which can take the ingest over
int fin_pair_prepass_fuses(const FinDevIndex* ix);
int fin_stream_blocks_per_cu(void);
void fin_debug_dump_time(void);   // -DFIN_V3_TIME builds: per-segment wave-cycle shares to stderr
int fin_walk_blocks_per_cu(void);
uint32_t fin_v4_counter_words(void);
uint64_t fin_v4_queue_slots(uint32_t n_reads, uint32_t max_grid_blocks);
uint64_t fin_v4_list_slots(uint32_t n_reads, uint32_t max_grid_blocks);
uint64_t fin_v4_workspace_bytes(uint32_t n_reads, uint32_t max_grid_blocks);
// kernel 4 = the pipeline probe -> route -> (stream -> walk) x rounds -> kernel 3 on what is left (fin_kernel_w.hip)
int fin_launch_search_v4(const FinDevIndex* ix, const uint8_t* bases, const void* packed, const FinReadDesc* desc,
                         const uint64_t* offs, const uint64_t* out_offs, void* out, uint64_t n_kmers, uint32_t n_reads,
                         int strands, uint32_t lds_deque_limit, uint32_t* ovf_list, uint32_t* ovf_count,
                         uint64_t* ovf_scratch, uint32_t ovf_blocks, uint32_t* pass, uint32_t* seed /* as pass, or NULL */, void* ws /* fin_v4_workspace_bytes */, uint64_t q_slots /* fin_v4_queue_slots */,
                         uint32_t* ctr /* fin_v4_counter_words() u32 */, uint32_t grid_probe, uint32_t grid_stream, uint32_t grid_walk, uint32_t grid_v3,
                         hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev_mid,
                         hipEvent_t out_ready /* NULL: the launcher prefills the output itself; else the prefill is done when this event fires */,
                         int no_prefill /* 1 (only if fin_v4_writes_gaps): nobody prefills, the pipeline writes every slot itself */,
                         uint32_t rounds /* stream / walk rounds to launch, 1 .. fin_v4_max_rounds() */,
                         int fused_ingest /* 1: no pack kernel, the pair pre-pass's fast kernel ingests `bases` (fin_launch_pair_prepass) */);
uint32_t fin_v4_max_rounds(void);
int fin_v4_writes_gaps(const FinDevIndex* ix, const uint32_t* seed);
int fin_probe_blocks_per_cu(void);
// fills the prefix table of depth T (4^T entries) from the uploaded node blocks
int fin_launch_build_ptab(const FinDevIndex* ix, void* tab, int T, hipStream_t stream);
// fills the anchor table pos[n_nodes + 1] (FinDevIndex::pos) and the safe-place bitmap safe[fin_anchor_safe_words()] (FinDevIndex::safe)
// from the uploaded index (fin_kernel_b.hip); tmp: fin_anchor_tmp_bytes() of device scratch; *n_unsafe: k-mer positions of the text that
// are not the place the reference reports for their k-mer (0: the bitmap is all ones and can be dropped).  Synchronises the stream.
uint64_t fin_anchor_safe_words(uint64_t total_len);
uint64_t fin_anchor_tmp_bytes(uint64_t total_len);
// kt3 (may be null; k <= 63): the compact k-mer table, kt3_buckets buckets of 32 bytes, filled by the same pass
int fin_launch_build_anchors(const FinDevIndex* ix, struct FinSeedEntry* pos, void* safe, void* kt3, uint32_t kt3_buckets, void* tmp, uint64_t* n_unsafe, hipStream_t stream, uint64_t* n_unver);
// the k-mers with an unverified answer, listed by that pass inside tmp (room for fin_anchor_ulist_cap() of them), and the exact side table made from the list
uint32_t fin_anchor_ulist_cap(uint64_t total_len);
void* fin_anchor_ulist(void* tmp, uint64_t total_len);
int fin_launch_build_ktx(const void* ulist, uint32_t n, void* ktx, uint32_t log2, hipStream_t stream);
// counts the k-mers of the text whose reverse complement is in the index too (fin_kernel_b.hip); tmp8: 8 bytes of device scratch.  Synchronises.
uint64_t fin_rcwin_bytes(uint64_t total_len);
int fin_launch_count_rc_pairs(const FinDevIndex* ix, void* tmp8, uint64_t* n_pairs, void* rcwin, hipStream_t stream);
// fills the canonical string filter (FinDevIndex::cbf; fin_kernel_b.hip): 2^log2_blocks blocks of 16 bytes over the unitigs' strings of m bases (m <= 32)
// (words_f, may be NULL: the directional filter FinDevIndex::fbf, same size, filled by the same pass)
int fin_launch_build_cbf(const FinDevIndex* ix, void* words, void* words_f, uint32_t log2_blocks, uint32_t m, hipStream_t stream);
// fills the absence filter filt[4^F / 32 + 8] (FinDevIndex::filt) from the uploaded text
int fin_launch_build_filter(const FinDevIndex* ix, uint32_t* filt, int F, hipStream_t stream);
int fin_launch_count_positive(const void* out, uint64_t n_pairs, unsigned long long* d_result, hipStream_t stream);
// index sets: a part's pairs into the set's result, unitigs renumbered by gid[] (fin_records.hip)
int fin_launch_set_merge(void* dst, const void* src, const uint32_t* gid, uint64_t n_pairs, int first, hipStream_t stream);
uint32_t fin_overflow_deque_cap(void);
// the reference's output text on the device (fin_text.hip)
uint32_t fin_text_blocks(uint64_t n_pairs);
uint64_t fin_text_off_words(uint64_t n_pairs);   // u64 words of d_blk_off
int fin_launch_text_lengths(const void* pairs, uint64_t n_pairs, const uint64_t* out_offs, uint32_t n_reads, uint32_t* d_last_bits,
                            uint32_t* d_blk_sum, uint64_t* d_blk_off, uint64_t* d_total, hipStream_t stream);
int fin_launch_text_write(const void* pairs, uint64_t n_pairs, const uint64_t* d_blk_off, const uint32_t* d_last_bits, char* d_text, hipStream_t stream);
uint64_t fin_text3_off_words(uint64_t n_seg);
uint32_t fin_text3_seg_pairs(void);
int fin_launch_text3_lengths(const void* pairs, const uint64_t* out_offs, const void* frec, const void* seg, uint32_t n_seg, uint32_t k,
                             uint32_t* d_seg_sum, uint64_t* d_seg_off, uint64_t* d_total, unsigned long long* d_found, hipStream_t stream);
int fin_launch_text3_write(const void* pairs, const uint64_t* out_offs, const void* frec, const void* seg, uint32_t n_seg, uint32_t k,
                           const uint64_t* d_seg_off, char* d_text, hipStream_t stream);
// diagnostic: the compact k-mer table asked about n k-mers {k0[i], k1[i]}: out[i] = {g, flags} (fin_kernels.hip)
int fin_launch_kt3_query(const FinDevIndex* ix, const uint64_t* k0, const uint64_t* k1, uint32_t n, void* out, hipStream_t stream);
// fin_records.hip: the pairs of the reads whose fast-path record stayed zero gathered into one dense stream (read order kept), their records stamped with nk
uint32_t fin_rec_blocks(uint32_t n_reads);
int fin_launch_rec_count(const void* frec, const uint64_t* out_offs, uint32_t n_reads, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, hipStream_t stream);
int fin_launch_rec_compact(void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, const uint64_t* blk_off, void* stream_out, hipStream_t stream);
// fin_hits.hip: counts[u] += the found k-mers of a finished step per unitig.  frec (null: the step left none -- the pair array is scanned end to end): the fast
// path's records, read as they stand (kind 1: one number per read; kind 0: the read's pairs through out_offs; kind 2: nothing).  flags: one u32 of the
// accumulator (bit 0: the step's overflow list overran -- nothing added; bit 1: a unitig number >= n_unitigs met -- not added).  combine: option "hits_combine"
int fin_launch_hits_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint64_t n_pairs, uint32_t k, void* counts,
                        uint32_t n_unitigs, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t combine, hipStream_t stream);
// fin_cover.hip: bits[ends_p[u] + off] |= 1 for every found pair (u, off) of a finished step -- one bit per base of the unitig text, uint64 words.  frec / out_offs /
// pairs / ovf_count / ovf_cap as fin_launch_hits_add.  flags: one u32 of the accumulator (bit 0: the step's overflow list overran -- nothing set; bit 1: a unitig
// number >= n_unitigs or a position >= total_len met -- skipped).  probe: option "cover_probe" (load the word first, skip the atomic OR when nothing would change)
int fin_launch_cover_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint64_t n_pairs, uint32_t k, const uint32_t* ends_p,
                         uint32_t n_unitigs, uint64_t total_len, void* bits, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t probe,
                         hipStream_t stream);
// covered[u] = popcount of unitig u's stretch of the bitmap (uint64[n_unitigs], zeroed here on `stream`)
int fin_launch_cover_count(const void* bits, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, void* covered, hipStream_t stream);
// fin_depth.hip: diff[g_lo] += 1, diff[g_hi + 1] -= 1 for every straight stretch of found places [g_lo, g_hi] of a finished step -- int32 diff[total_len + 1], the
// difference array of the per-position depth.  frec / out_offs / pairs / ovf_count / ovf_cap as fin_launch_hits_add.  flags: one u32 of the accumulator (bit 0: the
// step's overflow list overran -- nothing added; bit 1: a slot with a unitig number >= n_unitigs or a place >= total_len met -- it counts as absent)
int fin_launch_depth_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint64_t n_pairs, uint32_t k, const uint32_t* ends_p,
                         uint32_t n_unitigs, uint64_t total_len, void* diff, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream);
// the prefix sum of one chunk of the difference array: depth[0 .. n) = *carry + diff[0] + ... + diff[i]; n <= tile * fin_depth_max_chunk_tiles(),
// 1 <= tile <= fin_depth_max_tile(); tile_sum: a u32 per tile of the chunk; *carry moves on to the chunk's end.  Three kernels, none waits for another block
uint32_t fin_depth_max_tile(void);
uint32_t fin_depth_max_chunk_tiles(void);
int fin_launch_depth_scan_chunk(const void* diff, uint64_t n, uint32_t tile, uint32_t* tile_sum, uint32_t* carry, uint32_t* depth, hipStream_t stream);
// stats[u] += {sum, max, positions with depth >= min_depth} (FinDepthStat, zeroed by the caller) over depth[0 .. n), the depths of text positions g_base ..
int fin_launch_depth_stats(const uint32_t* depth, uint64_t g_base, uint64_t n, const uint32_t* ends_p, uint32_t n_unitigs, uint32_t min_depth, void* stats,
                           hipStream_t stream);
// fin_pileup.hip: the base pileup of a finished step -- alt uint32[total_len][4], diff int32[total_len + 1] (cover's difference array), counters
// 4 x u64 {kept, not straight, off the unitig, too many mismatches}, flags one u32 (bit 0: the step's overflow list overran -- nothing added; bit 1: a slot or record
// outside the index).  frec / out_offs / pairs / ovf_count / ovf_cap as fin_launch_hits_add; bases / offs: the batch's ASCII reads and their n_reads + 1 offsets;
// concat: the replica's 2-bit text
int fin_launch_pileup_add(const void* frec, const uint64_t* out_offs, const void* pairs, const uint8_t* bases, const uint64_t* offs, uint32_t n_reads, uint32_t k,
                          const uint32_t* ends_p, const uint32_t* concat, uint32_t n_unitigs, uint64_t total_len, uint32_t max_mismatch, void* alt, void* diff,
                          void* counters, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream);
// the call over one staged chunk -- cover[0 .. n) and alt[0 .. n) are text positions g_base .. g_base + n: fin_launch_pileup_call_count leaves blk_sum (u32) and
// blk_off (u64), fin_pileup_call_blocks(n) entries each, and *total = the chunk's candidates; fin_launch_pileup_call_write, once out has room for them: the
// entries {u, off, cover, ref, alt[4]} of 32 bytes, ascending
uint32_t fin_pileup_call_blocks(uint64_t n);
int fin_launch_pileup_call_count(const uint32_t* cover, const void* alt, uint64_t n, uint32_t min_alt, uint32_t min_permille, uint32_t* blk_sum, uint64_t* blk_off,
                                 uint64_t* total, hipStream_t stream);
int fin_launch_pileup_call_write(const uint32_t* cover, const void* alt, uint64_t g_base, uint64_t n, uint32_t min_alt, uint32_t min_permille, const uint32_t* ends_p,
                                 const uint32_t* concat, uint32_t n_unitigs, const uint64_t* blk_off, void* out, hipStream_t stream);
// fin_segments.hip: a finished step's results as segments {u, off, slot, len} of 16 bytes, dense and in read order, delimited per read by seg_offs[n_reads + 1].
// frec / out_offs / pairs as fin_launch_hits_add.  fin_launch_sgm_count: cnt[n_reads] u32, blk_sum[fin_sgm_blocks()] u32, blk_off as many u64, *total the
// batch's segments; fin_launch_sgm_write, once segs has room for them: seg_offs and the segments
uint32_t fin_sgm_blocks(uint32_t n_reads);
int fin_launch_sgm_count(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, uint32_t* cnt, uint32_t* blk_sum,
                         uint64_t* blk_off, uint64_t* total, hipStream_t stream);
int fin_launch_sgm_write(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const uint32_t* cnt,
                         const uint64_t* blk_off, uint64_t* seg_offs, void* segs, hipStream_t stream);
// the one-block exclusive prefix of n_blk > 0 per-block counts and their total, both uint64 (fin_blk_scan_kernel, fin_records.hip: every dense output made from per-block counts shares it)
int fin_launch_blk_scan(const uint32_t* blk_sum, uint32_t n_blk, uint64_t* blk_off, uint64_t* total, hipStream_t stream);
// fin_readsum.hip: a finished step's results as one summary {n_found, n_segments, longest, span} of 16 bytes per read (sum[n_reads]).  frec / out_offs / pairs
// as fin_launch_hits_add.  The screen made from the summaries: fin_launch_screen_bits writes bits[(n_reads + 63) / 64] (uint64, bit r & 63 of word r >> 6: read r
// passes), blk_sum[fin_rsm_blocks()] u32, blk_off as many u64 and *total = the passing reads; fin_launch_screen_ids, once ids has room for them: their numbers,
// ascending
uint32_t fin_rsm_blocks(uint32_t n_reads);
int fin_launch_read_summaries(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, void* sum, hipStream_t stream);
int fin_launch_screen_bits(const void* sum, const uint64_t* out_offs, uint32_t n_reads, uint32_t min_found, uint32_t min_permille, int invert, uint64_t* bits,
                           uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, hipStream_t stream);
int fin_launch_screen_ids(const uint64_t* bits, const uint64_t* blk_off, uint32_t n_reads, uint32_t* ids, hipStream_t stream);
// fin_classify.hip: a finished step's results as one class {label, n_best, n_second, n_labelled} of 16 bytes per read (cls[n_reads]) under labels[n_unitigs]
// (uint32 each, 0xFFFFFFFF: no label).  frec / out_offs / pairs as fin_launch_hits_add; a unitig number at or above n_unitigs has no label.
// fin_launch_class_tally: reads[label] += 1 for every read the rule assigns, reads[n_labels] += 1 for every other one (uint64[n_labels + 1])
int fin_launch_classify(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const uint32_t* labels, uint32_t n_unitigs,
                        void* cls, hipStream_t stream);
int fin_launch_class_tally(const void* cls, const uint64_t* out_offs, uint32_t n_reads, uint32_t n_labels, uint32_t min_found, uint32_t min_permille,
                           uint32_t min_margin, uint64_t* reads, hipStream_t stream);
// fin_taxa.hip -- taxonomic classification over parent[n_taxa] in topological numbering (fin_taxa.h).
// fin_launch_taxa_labels: label[u] = the LCA of the taxa of unitig u's colours (uint32[n_unitigs]; color_taxon on the device);
// fin_launch_taxa_reads: fin_read_taxon[n_reads], 16 bytes each, by Kraken's rule with the thresholds applied (frec null: every read's pairs are scanned);
// fin_launch_taxa_tally: direct[taxon] += 1 / direct[n_taxa] += 1 per read (uint64[n_taxa + 1]); fin_launch_taxa_clades: clade[n_taxa], zeroed by the caller, += direct over the subtrees
int fin_launch_taxa_labels(const uint64_t* bits, uint32_t W, uint32_t n_unitigs, const uint32_t* color_taxon, const uint32_t* parent, uint32_t* label, hipStream_t stream);
int fin_launch_taxa_reads(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const uint32_t* labels, uint32_t n_unitigs,
                          const uint32_t* parent, uint32_t min_found, uint32_t conf, void* out, hipStream_t stream);
int fin_launch_taxa_tally(const void* rt, uint32_t n_reads, uint32_t n_taxa, uint64_t* direct, hipStream_t stream);
int fin_launch_taxa_clades(const uint64_t* direct, const uint32_t* parent, uint32_t n_taxa, uint64_t* clade, hipStream_t stream);
// fin_colors.hip -- colour sets per unitig: bits uint64[n_unitigs * W], then one flag word (bit 0: a step whose overflow list overran was offered).
// fin_launch_colors_add: bit `color` for every unitig in which the step found a k-mer (frec null: every read's pairs are scanned).
// fin_launch_pseudoalign: rows uint64[n_reads * W] and heads {n_found, n_coloured, popcount, 0} per read under the threshold permille
int fin_launch_colors_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, void* bits, uint32_t W, uint32_t n_unitigs,
                          uint32_t color, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream);
int fin_launch_pseudoalign(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const void* bits, uint32_t W,
                           uint32_t n_unitigs, uint32_t permille, void* rows, void* heads, hipStream_t stream);
// fin_paired.hip -- one colour row per FRAGMENT (reads 2f and 2f + 1 of the step): rows uint64[n_frags * W] and heads {n_found, n_coloured, popcount,
// n_coloured of the first mate} under the threshold permille; mode 0: any mate, 1: the row is zero unless both mates have a coloured slot
int fin_launch_pseudoalign_paired(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_frags, uint32_t k, const void* bits, uint32_t W,
                                  uint32_t n_unitigs, uint32_t permille, uint32_t mode, void* rows, void* heads, hipStream_t stream);
// fin_fragments.hip -- the geometry of every FRAGMENT (reads 2f and 2f + 1 of the step): frags {u, start, length, cls} of 16 bytes each (may be
// null), and hist uint64[n_bins] += the inward fragments by min(length / bin_width, n_bins - 1), counters 7 x u64 += {the six classes, the inward lengths' sum}
// (both null: nothing is accumulated; n_bins <= 4096).  flags one u32, never null (bits as fin_launch_pileup_add); ends_p: the replica's unitig bounds
int fin_launch_fragments(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_frags, uint32_t k, const uint32_t* ends_p, uint32_t n_unitigs,
                         uint32_t n_bins, uint32_t bin_width, void* frags, void* hist, void* counters, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap,
                         hipStream_t stream);
// fin_links.hip -- the LINKS of a step (include/finito_amd.h: LINKS).  tab: cap slots of {u64 key, u64 count}, cap a power of two >= 4, then the
// trailer u64 n_distinct | u32 flags | u32 0 (FIN_LINKS_TRAILER bytes).  fin_launch_links_clear empties all of it; fin_launch_links_add inserts the step's
// transitions (a lane per read; only kind-0 reads are scanned); ends_p: the replica's unitig bounds
#define FIN_LINKS_TRAILER 16u
int fin_launch_links_clear(void* tab, uint32_t cap, hipStream_t stream);
int fin_launch_links_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len,
                         void* tab, uint32_t cap, uint64_t max_links, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream);
// the download's passes on the table as it stands.  Count: blk_sum[fin_links_blocks(cap)] = the slots per block of 256 with count >= min_count (>= 1), blk_off and
// *total their exclusive prefix and sum (fin_launch_blk_scan), stats u64[2] += {the sum of all counts, the occupied slots whose two places are equal} (zeroed
// by the caller).  Write: out[d] = the d-th such slot as fin_link, in slot order, its ends found by binary search in ends_p
uint32_t fin_links_blocks(uint32_t cap);
int fin_launch_links_count(const void* tab, uint32_t cap, uint64_t min_count, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, uint64_t* stats, hipStream_t stream);
int fin_launch_links_write(const void* tab, uint32_t cap, uint64_t min_count, const uint64_t* blk_off, const uint32_t* ends_p, uint32_t n_unitigs, void* out,
                           hipStream_t stream);
// ... over a COMPACT matrix (fin_colorsets.hip's state): sets uint64[(n_sets + 1) * W] with row 0 empty, set_of uint32[n_unitigs], each <= n_sets.  A unitig number
// becomes its set id as it is loaded, the register table is keyed by set id; the results are those of the dense launch over the expanded matrix, bit for bit
int fin_launch_pseudoalign_sets(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const void* sets, uint32_t W, uint32_t n_sets,
                                const uint32_t* set_of, uint32_t n_unitigs, uint32_t permille, void* rows, void* heads, hipStream_t stream);
int fin_launch_pseudoalign_paired_sets(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_frags, uint32_t k, const void* sets, uint32_t W,
                                       uint32_t n_sets, const uint32_t* set_of, uint32_t n_unitigs, uint32_t permille, uint32_t mode, void* rows, void* heads,
                                       hipStream_t stream);
// fin_colorsets.hip -- the distinct rows of a colour matrix, each once.  fin_launch_cs_claim: slots (2^lg u64, lg 1 .. 27) and ctr (4 u64: slots claimed, rows that
// met a foreign row under their tag, the longest probe, flags -- bit 0: the table or max_sets overran) zeroed by the caller; slot_of n_unitigs u32; blk_sum
// fin_cs_blocks(2^lg) u32, blk_off as many u64, *total = n_sets.  tag_bits: option "colorsets_tag_bits".  Once the host has read ctr and *total:
// fin_launch_cs_gather writes sets ((n_sets + 1) rows of W words, row 0 zero) and set_of (n_unitigs u32); slot_id: 2^lg u32 of scratch.
// fin_launch_cs_expand: bits[u] = sets[set_of[u]]
uint32_t fin_cs_blocks(uint32_t slots);
int fin_launch_cs_claim(const void* bits, uint32_t n_unitigs, uint32_t W, void* slots, uint32_t lg, uint32_t tag_bits, uint64_t max_sets, uint32_t* slot_of, void* ctr,
                        uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, hipStream_t stream);
int fin_launch_cs_gather(const void* bits, uint32_t n_unitigs, uint32_t W, const void* slots, uint32_t lg, const uint32_t* slot_of, const uint64_t* blk_off,
                         uint32_t* slot_id, void* sets, uint32_t* set_of, hipStream_t stream);
int fin_launch_cs_expand(const uint32_t* set_of, const void* sets, uint32_t n_unitigs, uint32_t W, void* bits, hipStream_t stream);
// fin_eqclasses.hip -- equivalence classes of colour rows: an open-addressing table of 2^lg slots (tags, counts: a u64 per slot; tab_rows: W u64 per slot; ctr:
// 8 u64 -- rows added, unaligned, classes, rows through the serial pass, flags, the collision list's length).  fin_launch_ec_add: rows uint64[n_rows * W] are added
// in three launches (claim, verify and count, collisions serially); slot_of and coll: n_rows u32 of scratch each.  tag_bits / combine: options "ec_tag_bits" and
// "ec_combine".  fin_launch_ec_occupied + fin_launch_ec_gather: the occupied slots as a dense {row, reads} list in slot order
int fin_launch_ec_add(const void* rows, uint32_t n_rows, uint32_t W, uint32_t n_colors, void* tags, void* counts, void* tab_rows, uint32_t lg, uint64_t max_classes,
                      uint32_t tag_bits, uint32_t combine, void* ctr, uint32_t* slot_of, uint32_t* coll, hipStream_t stream);
// the weighted add: row r counts weights[r] times (uint64[n_rows]; 0: skipped, no class), n_unaligned all-zero rows besides; no combine
int fin_launch_ec_add_classes(const void* rows, const void* weights, uint32_t n_rows, uint64_t n_unaligned, uint32_t W, uint32_t n_colors, void* tags, void* counts,
                              void* tab_rows, uint32_t lg, uint64_t max_classes, uint32_t tag_bits, void* ctr, uint32_t* slot_of, uint32_t* coll, hipStream_t stream);
uint32_t fin_ec_blocks(uint32_t slots);
int fin_launch_ec_occupied(const void* tags, uint32_t slots, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, hipStream_t stream);
int fin_launch_ec_gather(const void* tags, const void* counts, const void* tab_rows, uint32_t slots, uint32_t W, const uint64_t* blk_off, void* out_rows,
                         void* out_reads, hipStream_t stream);
// fin_abundance.hip -- EM over the dense class list fin_launch_ec_gather leaves (rows uint64[C][W], reads uint64[C]).  FinAbState is the device-side
// word the kernels stop on: zeroed before iteration 0, written by an iteration's last kernel.  fin_ab_geometry: the launch geometry of an estimate -- classes per
// block of the first pass and its blocks, classes per chunk of the column pass and its chunks -- a function of C, W and option "ab_chunk" (0: auto) alone, which
// is what the fixed order of every sum rests on.  fin_launch_ab_transpose: rowsT[W][C] from rows[C][W].  fin_launch_ab_iteration: iteration t in four launches
// (x, alpha, len: 64 W doubles; q: C; part: n_chunks * 64 W; ll_part: n_ll; blk_ok: 64 u32; blk_chg: 64; trace: a double per iteration enqueued); it changes
// nothing once state->done is set
typedef struct FinAbState { uint32_t done, iters; double max_change, loglik; } FinAbState;
void fin_ab_geometry(uint64_t C, uint32_t W, uint32_t ab_chunk, uint32_t* cpb, uint32_t* n_ll, uint32_t* chunk, uint32_t* n_chunks);
int fin_launch_ab_transpose(const void* rows, uint64_t C, uint32_t W, void* rowsT, hipStream_t stream);
int fin_launch_ab_iteration(void* state, const void* rows, const void* rowsT, const void* reads, uint64_t C, uint32_t W, uint32_t n_colors, uint32_t ab_chunk,
                            const double* len, double n_total, double tol, double* alpha, double* x, double* q, double* part, double* ll_part, uint32_t* blk_ok,
                            double* blk_chg, uint32_t t, double* trace, hipStream_t stream);
// fin_bootstrap.hip -- a bootstrap replicate's class counts, drawn over the same dense list (the draws: fin_bootrng.h).  fin_launch_ab_rowhash:
// h[C], the rows' 64-bit hashes.  fin_launch_ab_slabs: slabs[C] (uint32, ceil(n_j / 4096); n_j < 2^40), their exclusive prefix[C] and *total.
// fin_launch_ab_resample: replicate b (< 4096) under `seed` -- counts[C] and *n_b, both zeroed by the caller before the launch; S: that total, read by the host
int fin_launch_ab_rowhash(const void* rows, uint64_t C, uint32_t W, void* h, hipStream_t stream);
int fin_launch_ab_slabs(const void* reads, uint64_t C, uint32_t* slabs, uint64_t* prefix, uint64_t* total, hipStream_t stream);
int fin_launch_ab_resample(const void* h, const void* reads, const uint64_t* prefix, uint64_t C, uint64_t S, uint64_t seed, uint32_t b, void* counts, void* n_b,
                           hipStream_t stream);
// fin_assign.hip -- rows assigned to colours from per-colour weights: rows uint64[n_rows * W] in HBM; x, thr: 64 W doubles each (0 behind n_colors);
// out_rows uint64[n_rows * W] and heads {n_assigned, best} of 8 bytes per row (either may be null); assigned, sole: uint64[n_colors]; counters: 4 uint64 {rows,
// unaligned, unassigned, multi} -- all three added to with integer atomics.  assign_rpb: option "assign_rpb"; fin_assign_rpb: the rows a block then takes.
// fin_launch_assign_column: bit `color` of every assigned row as the bitmap, block sums, block offsets and total that fin_launch_screen_ids takes
uint32_t fin_assign_rpb(uint64_t n_rows, uint32_t assign_rpb);
// (fin_assign_host.cpp, no device) the first colour whose weight is negative, NaN or infinite (*what = 0) or whose threshold is outside [0, 1] or NaN (*what = 1); n_colors: none
uint32_t fin_assign_first_bad(const double* weights, const double* thresholds, uint32_t n_colors, int* what);
int fin_launch_assign_rows(const void* rows, uint64_t n_rows, uint32_t W, uint32_t n_colors, uint32_t assign_rpb, const double* x, const double* thr, void* out_rows,
                           void* heads, uint64_t* assigned, uint64_t* sole, uint64_t* counters, hipStream_t stream);
int fin_launch_assign_column(const void* arows, uint32_t n_rows, uint32_t W, uint32_t color, uint64_t* bits, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total,
                             hipStream_t stream);
// fin_colcov.hip -- the per-unitig coverage numbers projected through the colour matrix: bits uint64[n_unitigs * W]; ends_p, total_len and k give
// nk(u); covered uint64[n_unitigs] and stats FinDepthStat[n_unitigs] (either may be null: zeros); cls: n_unitigs bytes the launcher fills (0 empty row, 1 one
// colour, 2 more).  out uint64[n_colors][8] {kmers, kmers_only, covered, covered_only, depth_sum, depth_sum_only, solid, solid_only} and none uint64[8] (the
// unitigs without a colour; its _only places stay 0), both zeroed on `stream` by the launcher.  colcov_chunk: option "colcov_chunk"; fin_colcov_chunk: the
// unitigs a wave then takes.  loads: 0 coalesced slices broadcast through the wave (the library's), 1 wave-uniform loads (kept for tools/ab_colcov.py)
uint32_t fin_colcov_chunk(uint64_t n_unitigs, uint32_t W, uint32_t colcov_chunk);
int fin_launch_color_coverage(const void* bits, uint32_t n_unitigs, uint32_t W, uint32_t n_colors, const uint32_t* ends_p, uint64_t total_len, uint32_t k,
                              const void* covered, const void* stats, void* cls, uint32_t colcov_chunk, uint32_t loads, uint64_t* out, uint64_t* none,
                              hipStream_t stream);
// fin_colsim.hip -- the colour matrix times itself under a weight per unitig: out uint64[n_colors][n_colors], out[i][j] = the sum of v(u) over the
// unitigs whose row has bits i and j, mod 2^64, the full symmetric matrix, zeroed on `stream` by the launcher.  vals uint64[n_unitigs], or null: nk(u) from
// ends_p, total_len and k.  colsim_chunk: option "colsim_chunk"; fin_colsim_chunk: the unitigs a wave then takes
uint32_t fin_colsim_chunk(uint64_t n_unitigs, uint32_t W, uint32_t colsim_chunk);
int fin_launch_color_shared(const void* bits, uint32_t n_unitigs, uint32_t W, uint32_t n_colors, const uint32_t* ends_p, uint64_t total_len, uint32_t k,
                            const void* vals, uint32_t colsim_chunk, uint64_t* out, hipStream_t stream);
// ... the class byte alone (fin_colcov_class_kernel unchanged): cls n_unitigs bytes; none8: eight uint64 of device scratch, zeroed and written here, not a result
int fin_launch_color_classes(const void* bits, uint32_t n_unitigs, uint32_t W, const uint32_t* ends_p, uint64_t total_len, uint32_t k, void* cls, uint64_t* none8,
                             hipStream_t stream);
// fin_depthhist.hip -- depth histograms over the staged depths of fin_launch_depth_scan_chunk: bin(d) = min(d / bin_width, n_bins - 1), 1 <= n_bins <=
// fin_depthhist_max_bins() = 1024, bin_width >= 1; a position counts iff a k-mer begins there (g + k <= the end of its unitig).  depth[0 .. n) are the depths of text
// positions g_base .. g_base + n, 16-byte aligned.  fin_launch_depth_spectrum: hist uint64[n_bins], zeroed by the caller, += the chunk's spectrum.
// fin_launch_color_depth_hist: one sub-range of unitigs [u_lo, u_hi) of the chunk, whose positions are the window [lo, hi) of the stage (fewer than 2^32): V
// uint32[(u_hi - u_lo) * n_bins] is zeroed and binned, then projected through bits uint64[n_unitigs * W] under the class bytes cls: out uint64[n_colors][2][n_bins]
// {all, only} and none uint64[n_bins] are added to (the caller zeroes them before the first sub-range).  variant: 0 = lane per colour, the only projection built
uint32_t fin_depthhist_max_bins(void);
int fin_launch_depth_spectrum(const uint32_t* depth, uint64_t g_base, uint64_t n, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, uint32_t k,
                              uint32_t n_bins, uint32_t bin_width, uint64_t* hist, hipStream_t stream);
int fin_launch_color_depth_hist(const uint32_t* depth, uint64_t g_base, uint64_t n, uint64_t lo, uint64_t hi, const uint32_t* ends_p, uint32_t n_unitigs,
                                uint64_t total_len, uint32_t k, uint32_t n_bins, uint32_t bin_width, uint32_t u_lo, uint32_t u_hi, uint32_t* V, const void* bits,
                                uint32_t W, uint32_t n_colors, const void* cls, uint32_t variant, uint64_t* out, uint64_t* none, hipStream_t stream);
// fin_refpaths.hip -- reference coordinates: segs fin_segment[n_segs] of n_seqs sequences delimited by seg_offs[n_seqs + 1], both in HBM.
// fin_rp_tile: the slots a wave's tile holds under option "refpaths_tile" (0: auto).  fin_launch_rp_tiles: cnt n_segs u32, blk_sum fin_rp_blocks() u32, blk_off as
// many u64, tile_offs[n_segs + 1] u64 and *total = the tiles.  fin_launch_rp_depth, once the host has read *total: win {u64 depth_sum, u32 in_graph, u32 covered} per
// window, zeroed by the caller, win_offs[n_seqs + 1] the sequences' first windows, depth uint32[total_len]; flags one u32 (bit 1: a segment outside the index or
// outside its sequence's windows -- it added nothing).  fin_launch_rp_var_g: g[n] = the text positions of fin_variant vars[n].  fin_launch_rp_var_count /
// fin_launch_rp_var_write: the variants inside every segment's base interval as records {seq, pos, var, flags} of 16 bytes, by segment, then by pos; out has room for
// *total of them
uint32_t fin_rp_tile(uint32_t refpaths_tile);
uint32_t fin_rp_blocks(uint64_t n_segs);
int fin_launch_rp_tiles(const void* segs, uint64_t n_segs, uint32_t tile, uint32_t* cnt, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* tile_offs, uint64_t* total,
                        hipStream_t stream);
int fin_launch_rp_depth(const void* segs, uint64_t n_segs, const uint64_t* seg_offs, uint64_t n_seqs, const uint64_t* tile_offs, uint64_t n_tiles, uint32_t tile,
                        const uint64_t* win_offs, uint32_t window, uint32_t min_depth, const uint32_t* depth, const uint32_t* ends_p, uint32_t n_unitigs,
                        uint64_t total_len, uint32_t k, void* win, uint32_t* flags, hipStream_t stream);
int fin_launch_rp_var_g(const void* vars, uint64_t n, const uint32_t* ends_p, uint64_t* g, hipStream_t stream);
int fin_launch_rp_var_count(const void* segs, uint64_t n_segs, const uint64_t* g, uint64_t n_vars, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len,
                            uint32_t k, uint32_t* cnt, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, uint32_t* flags, hipStream_t stream);
int fin_launch_rp_var_write(const void* segs, uint64_t n_segs, const uint64_t* seg_offs, uint64_t n_seqs, const uint64_t* g, uint64_t n_vars, const uint32_t* ends_p,
                            uint32_t n_unitigs, uint64_t total_len, uint32_t k, const uint64_t* blk_off, void* out, uint32_t* flags, hipStream_t stream);
#ifdef __cplusplus
}
#endif
