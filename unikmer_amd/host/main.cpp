// main.cpp — `unikmer`-compatible command line driver over the C ABI of libunikmer_hip.so: the dispatch.
//
// The reference's L3/L4 layers (the cobra sub-commands of unikmer/cmd/*.go) are
// Go; the build has no Go toolchain, so the host side of the drop-in is C++ (the
// INTEGRATION.md cgo shim documents the Go binding).  Commands keep the reference's names,
// flags and output-naming rules; all k-mer arithmetic that the reference does per record on
// the CPU goes through the HIP library.  One translation unit, in layers:
//   base.hpp, seqtext.hpp   device-free: errors, flags, paths, k-mer text, the FASTA/Q parser (tests/host_units.cpp)
//   count_pipe.hpp          device-free: the chunk pipeline of count -- the pipe between the reader thread and the device thread,
//                           the handover of a file to the host parser, the reader bodies, the double-buffered loop
//                           (tests/count_pipe_units.cpp)
//   records.hpp             .unik files <-> host vectors <-> library calls: the input loader and the shared steps
//   cmd_count.hpp   count  (count.go)   FASTA/Q -> [ukm_fastx ->] ukm_encode_kmers | ukm_nthash | ukm_minimizer -> ukm_sort_* ->
//                          ukm_unique; the window values stay on the device from encode to the final set.  A CountJob, the two
//                          stages of count_pipe.hpp's loop (ParsedStage, RawStage), finish_count; count_on_device wires them
//   cmd_setops.hpp  union / inter / diff / common -> ukm_union_ft / ukm_inter_ft / ukm_diff_ft / ukm_common_ft
//   cmd_chunks.hpp  sort   (sort.go)    ukm_sort_u64 | ukm_sort_pairs -> ukm_unique(-u/-d); with -m, and for split / merge,
//                          the chunk protocol: sorted chunk files -> ukm_merge_k_ft
//   cmd_map.hpp     locate (locate.go)  genome FASTA + .unik codes -> ukm_locate -> BED6
//                   map / uniqs (map.go, -x 0 -X 0, linear)  .unik files -> ukm_union -> per genome file ukm_map -> BED3 | FASTA
//   cmd_select.hpp  grep / filter / sample (grep.go, filter.go, sample.go)  per input file ukm_grep | ukm_filter | ukm_sample: the kept
//                          records in input order with their own taxids; grep -s/-u/-d -> ukm_sort_* -> ukm_unique
//                   rfilter (rfilter.go)  nodes.dmp with ranks + rank file -> ukm_taxonomy_set_ranks; per input file ukm_rfilter
//                   tsplit  (tsplit.go)   the files' records with their taxids -> ukm_tsplit -> one .unik per taxid
//   cmd_cpu.hpp     commands that need no GPU: view, dump, num, info/stats, concat, head, encode, decode; where there is one,
//                          dump (without -H) parses its text with ukm_dump and view (without -g, under UNIKMER_DEVICE_TEXT=1)
//                          renders its text with ukm_view
// .unik bodies are decoded and encoded by ukm_unik_decode / ukm_unik_encode (records.hpp) unless UNIKMER_HOST_CODEC=1;
// UNIKMER_HOST_TEXT=1 keeps view and dump on their host loops.
// Not implemented (SURVEY.md §2a out of scope): grep -m/-O/-S/--force, rfilter's built-in default rank list,
// map -x/-X/--circular, autocompletion; count -S (syncmer sketch: third-party rule not reconstructable from the tree).
#include "cmd_chunks.hpp"
#include "cmd_count.hpp"
#include "cmd_cpu.hpp"
#include "cmd_map.hpp"
#include "cmd_select.hpp"
#include "cmd_setops.hpp"

static const char *VERSION = "0.21.0-hip";

static void usage() {
    fprintf(stderr,
            "unikmer (HIP) - k-mer set operations on AMD MI355X behind the unikmer command line\n\n"
            "Usage: unikmer <command> [flags] [files]\n\n"
            "GPU commands : count sort split merge union inter diff common locate map(uniqs) grep filter sample rfilter tsplit\n"
            "CPU commands : view dump num info(stats) concat head encode decode version\n"
            "Global flags : -j --verbose -C --compression-level -c -i -I --max-taxid --data-dir --gpu\n");
}

int main(int argc, char **argv) {
    if (argc < 2) { usage(); return 0; }
    const string cmd = argv[1];
    argc -= 2; argv += 2;
    try {
        if (cmd == "count") return cmd_count(argc, argv);
        if (cmd == "sort") return cmd_chunks(CH_SORT, argc, argv);
        if (cmd == "split") return cmd_chunks(CH_SPLIT, argc, argv);
        if (cmd == "merge") return cmd_chunks(CH_MERGE, argc, argv);
        if (cmd == "union") return cmd_setop(OP_UNION, argc, argv);
        if (cmd == "inter") return cmd_setop(OP_INTER, argc, argv);
        if (cmd == "diff") return cmd_setop(OP_DIFF, argc, argv);
        if (cmd == "common") return cmd_setop(OP_COMMON, argc, argv);
        if (cmd == "locate") return cmd_locate(argc, argv);
        if (cmd == "map" || cmd == "uniqs") return cmd_map(argc, argv);
        if (cmd == "grep") return cmd_grep(argc, argv);
        if (cmd == "filter") return cmd_filter(argc, argv);
        if (cmd == "sample") return cmd_sample(argc, argv);
        if (cmd == "rfilter") return cmd_rfilter(argc, argv);
        if (cmd == "tsplit") return cmd_tsplit(argc, argv);
        if (cmd == "view") return cmd_view(argc, argv);
        if (cmd == "dump") return cmd_dump(argc, argv);
        if (cmd == "num") return cmd_num(argc, argv);
        if (cmd == "info" || cmd == "stats") return cmd_info(argc, argv);
        if (cmd == "concat") return cmd_concat(argc, argv);
        if (cmd == "head") return cmd_head(argc, argv);
        if (cmd == "encode") return cmd_encode(argc, argv);
        if (cmd == "decode") return cmd_decode(argc, argv);
        if (cmd == "version") { printf("unikmer v%s\n", VERSION); return 0; }
        if (cmd == "-h" || cmd == "--help" || cmd == "help") { usage(); return 0; }
        die("unknown command \"%s\" for \"unikmer\"", cmd.c_str());
    } catch (const unik::Error &e) {
        die("%s", e.what());
    } catch (const std::exception &e) {
        die("%s", e.what());
    }
}
