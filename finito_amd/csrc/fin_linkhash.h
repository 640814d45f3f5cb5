// fin_linkhash.h -- the hash of the link table, for the device and the host alike (include/finito_amd.h: LINKS, fin_link_hash states the arithmetic): a key's
// home slot is fin_link_mix(key) & (cap - 1).  fin_links.hip probes with it, fin_links_host.cpp exports it as fin_link_hash, tests aim keys with it.
#pragma once
#include "fin_rec_walk.h"

#define FIN_LINK_EMPTY 0xFFFFFFFFFFFFFFFFull   // no place is 0xFFFFFFFF (total_len < 2^32), so no key is all ones

FIN_HD uint64_t fin_link_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// the unordered pair of two places
FIN_HD uint64_t fin_link_key(uint32_t ga, uint32_t gb) { return ga < gb ? ((uint64_t)ga << 32) | gb : ((uint64_t)gb << 32) | ga; }
