// oc2cns - drop-in replacement of NECAT's oc2cns (consensus/main.c:51-78):
//   oc2cns [options] wrk_dir candidates cns_out raw_out [-mn node_id num_nodes]
// Same argv (consensus/cns_options.c:10, -mn as consensus/main.c:37-41), same inputs (the volume directory, the
// candidate partitions `candidates.p<i>` written by oc2pcan), same two FASTA outputs: corrected reads / stretches
// (cns_out) and the uncorrected rest (raw_out), record format DUMP_CNS_SEQ (common/cns_seq.h:24-44).
//
// Per partition: the extension loop of every template runs on the GPU (necat_cns_extension_batch: which candidates get
// aligned, which alignments count, with what weight - consensus/consensus_one_read.c:221-372), the consensus proper
// (tasc/) through necat_cns_consensus_batch: on the library's host threads (cns_consensus.h; NECAT_CNS_DEVICE=0) or on the
// device with a certified fallback to that code (NECAT_CNS_DEVICE=1); the record text is written here.  Records come out in template order (the reference's order with -t 1;
// with more threads the reference's order depends on scheduling).
// -r 1 (rescue_long_indels): candidates whose block-wise extension failed or fell short go through DALIGNER's local alignment and
// edlib's global path after each device pass, as in the reference (cns_rescue.h): on the host threads, or on the device with
// NECAT_DALIGN_DEVICE=1 / NECAT_NW_DEVICE=1 (necat_local_align_batch / necat_nw_path_batch).  -s 1 (small memory: reads
// loaded per partition) behaves like -s 0 - the read set is resident in HBM either way.  There is no CPU fallback for the
// block-wise alignments: without a usable GPU the program exits 1.
// The job itself - the read set, merged or gathered per chunk of templates, the two stages and their hand-off - is cns_job.h; this file is the command line.
#include "cns_job.h"

using namespace necat_host;

namespace {

struct CnsOpts {             // consensus/cns_options.h:6-18, defaults cns_options.c:10-22
    int min_align_size = 400, min_cov = 4, max_cov = 12, min_size = 500, full_consensus = 0;
    double error = 0.5, mapping_ratio = 0.8;
    int num_threads = 1, rescue_long_indels = 0, use_fixed_ident_cutoff = 0, small_memory = 0;
};

void describe(FILE* out)
{
    fprintf(out, "-a <Integer>\talign length cutoff\n-x <Integer>\tminimal coverage\n-y <Integer>\tmaximal coverage\n"
                 "-l <Integer>\tminimal length of corrected reads.\n-f <0 or 1>\tfull consensus or not: 1 = yes, 0 = no\n"
                 "-e <Real>\tsequencing error\n-p <Real>\tminimal mapping ratio\n-t <Integer>\tnumber of cpu threads\n"
                 "-r <0 or 1>\trescue long indels or not: 1 = yes, 0 = no\n-u <0 or 1>\tuse dynamic or fixed ident cutoff: 1 = fixed, 0 = dynamic\n"
                 "-s <0 or 1>\tuse small memoty\nDEFAULT OPTIONS:\n");
    CnsOpts d;
    fprintf(out, "-a %d -x %d -y %d -l %d -f %d -e %f -p %f -t %d -r %d -u %d -s %d\t\n", d.min_align_size, d.min_cov, d.max_cov, d.min_size, d.full_consensus,
            d.error, d.mapping_ratio, d.num_threads, d.rescue_long_indels, d.use_fixed_ident_cutoff, d.small_memory);
}

bool parse(int argc, char** argv, CnsOpts* o)
{
    optind = 1;
    int c;
    while ((c = getopt(argc, argv, "a:x:y:l:f:e:p:t:r:u:s:")) != -1) {
        switch (c) {
        case 'a': o->min_align_size = atoi(optarg); break;
        case 'x': o->min_cov = atoi(optarg); break;
        case 'y': o->max_cov = atoi(optarg); break;
        case 'l': o->min_size = atoi(optarg); break;
        case 'f': o->full_consensus = atoi(optarg); break;
        case 'e': o->error = atof(optarg); break;
        case 'p': o->mapping_ratio = atof(optarg); break;
        case 't': o->num_threads = atoi(optarg); break;
        case 'r': o->rescue_long_indels = atoi(optarg); break;
        case 'u': o->use_fixed_ident_cutoff = atoi(optarg); break;
        case 's': o->small_memory = atoi(optarg); break;
        default: return false;
        }
    }
    return true;
}

int usage(const char* prog)
{
    fprintf(stderr, "USAGE:\n%s [options] wrk_dir candidates cns_out raw_out\n\nIf Multiple Nodes Are Used:\n"
                    "%s [options] wrk_dir candidates cns_out raw_out -mn node_id num_nodes\n\nOPTIONS AND DESCRIPTIONS:\n", prog, prog);
    describe(stderr);
    return 1;
}

int fail(const char* what, const char* detail) { fprintf(stderr, "[oc2cns] ERROR: %s: %s\n", what, detail); return 1; }

}  // namespace

int main(int argc, char** argv)
{
    necat_host::necat_cli_env();          // (before the first HIP call: host_io.h)
    CnsOpts opt;
    int spid = 0, nnode = 1;
    int ac = argc;
    if (ac >= 8 && strcmp(argv[ac - 3], "-mn") == 0) { spid = atoi(argv[ac - 2]); nnode = atoi(argv[ac - 1]); ac -= 3; }
    if (ac < 5 || !parse(ac - 4, argv, &opt) || nnode < 1 || spid < 0) return usage(argv[0]);
    if (opt.max_cov < 1 || opt.min_cov < 0) return fail("options", "coverage limits out of range");

    necat_cns_options co; necat_cns_default_options(&co);
    co.min_align_size = opt.min_align_size; co.min_cov = opt.min_cov; co.max_cov = opt.max_cov; co.error = opt.error;
    co.mapping_ratio = opt.mapping_ratio; co.use_fixed_ident_cutoff = opt.use_fixed_ident_cutoff;
    co.rescue_long_indels = opt.rescue_long_indels != 0;
    necat_cns_consensus_options cco; necat_cns_consensus_default_options(&cco);
    cco.min_cov = opt.min_cov; cco.min_size = opt.min_size; cco.full_consensus = opt.full_consensus != 0;
    cco.host_threads = std::max(1, std::min(opt.num_threads, 256));       // -t: host threads of the consensus proper (its host form and fallback) and of the record text
    return cns_run_job(co, cco, opt.small_memory != 0, argv[ac - 4], argv[ac - 3], argv[ac - 2], argv[ac - 1], spid, nnode, cli_device());
}
