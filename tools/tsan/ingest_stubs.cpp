// Stand-ins for what the host units of the ingest (hulk_ingest_gzip.hip, hulk_ingest_source.hip, hulk_ingest_host.hip) take from the
// rest of libhulkhip.so, so that hulk_parse_files alone (readers, gzip readers, block reader, parser; no GPU sink) links into a
// ThreadSanitizer build: tools/tsan_ingest.sh
#include "include/hulk_hip.h"
#include "hulk_amd/csrc/hulk_bgzf.h"
namespace hulk {
namespace bgzf {
// (the device BGZF reader is only opened when a run has device buffers for it — hulk_sketch_files; never here — but it has to link)
bool DevReader::looks_like(int) { return false; }
DevReader::DevReader(int fd, DevBufs *b, bool trace) : fd_(fd), b_(b), trace_(trace) {}
DevReader::~DevReader() {}
long DevReader::read(uint8_t *, size_t, uint8_t *, std::string &msg) { msg = "stub"; return -1; }
}
}
extern "C" {
const char *hulk_strerror(int) { return "error"; }
}
