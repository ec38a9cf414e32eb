// guide_table.h — host-side check of a guide's tables (include/bloomstage.h "Guided decoding").  No HIP: the check is
// plain C++ so that a stand-alone program can run it under the host sanitizers (tools/guide_table_check.cpp).
#pragma once
#include <string>

#include "bloomstage.h"

// true if `g` is a well-formed guide for a vocabulary of `vocab` entries; otherwise *msg says what is wrong and in
// which state.  Reads row_ptr[0 .. n_states], default_next[0 .. n_states) and the edge arrays up to row_ptr[n_states],
// and only as far as the entries read so far are consistent.
bool guide_table_check(const bs_guide_desc* g, int vocab, std::string* msg);
