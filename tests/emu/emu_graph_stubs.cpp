// TEST INFRASTRUCTURE ONLY -- the hipGraph entry points of the C ABI (csrc/runtime.hip is not part of the emulator build).
// They exist so that their binding can be inspected on the CPU tier; nothing calls them (an emulated library launches
// eagerly), and a call is refused.  Kept out of emu_runtime.cpp, which also links into the stand-alone scheduler self-test
// without common.cpp.
#include <errno.h>

#include "common.h"

static int refuse(const char* what) { return leco::fail(-ENOSYS, "%s: the host emulator has no hipGraph", what); }

extern "C" int leco_graph_begin_capture(leco_stream_t) { return refuse("leco_graph_begin_capture"); }
extern "C" int leco_graph_end_capture(leco_stream_t, leco_graph_t*) { return refuse("leco_graph_end_capture"); }
extern "C" int leco_graph_launch(leco_graph_t, leco_stream_t) { return refuse("leco_graph_launch"); }
extern "C" int leco_graph_destroy(leco_graph_t) { return refuse("leco_graph_destroy"); }
