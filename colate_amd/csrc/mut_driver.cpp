// colate_amd/csrc/mut_driver.cpp -- `Colate --mode mut` as a library call
// (colate_mut_main in include/colate_amd.h): the command line of the reference
// (include/coal/Colate.cpp:6-116) for the .colate.in / .colate_mat inputs, the
// feeder that turns two .colate.in streams and the .mut files into per-block
// age-bin tables (include/coal/coal.cpp:2071-2321 with include/src/mutations.cpp:56-283
// and include/src/data.cpp:213-235), and the mut() driver (include/coal/coal.cpp:3071-3863)
// around the GPU EM (colate_em_batch), for one pair (run_mut), for a `--pairs` list
// (run_mut_pairs; the tables of both come from the engine of mut_pairs.cpp) and for the
// pairs of a `--samples` list (run_mut_samples; the tables come from the walk and fill on
// the device, fill_samples.cpp).  The two lists share run_pair_list, everything behind the fill.
//
// Everything here runs once per invocation on the host; the per-replicate EM,
// which is where the reference spends its time, is the HIP kernel.
#include <fcntl.h>
#include <poll.h>
#include <sys/resource.h>
#include <sys/wait.h>
#include <unistd.h>
#include <zlib.h>

#include <signal.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "age_bins.hpp"
#include "colate_amd.h"
#include "colate_internal.h"
#include "mut_feeder.h"
#include "mut_interval.h"

namespace colate_drv {

// ------------------------------------------------------------------ options
// Same option names as Colate.cpp:11-45 (unknown options are an error there too:
// cxxopts throws option_not_exists_exception).  `--num_bootstrap` (README spelling)
// is accepted as an alias of `--num_bootstraps`.  Ours: `--device N` (GPU ordinal), `--devices N`
// (shard the replicates over GPUs 0..N-1 of the node from this one process), `--ranks N` (the same sharding as N
// processes, one per GPU, with one RCCL all-gather of the results: run_ranked below),
// `--counts_out FILE` (write the bootstrap count tables in the reference's .colate_mat layout,
// 17 significant digits), `--counts_only` (stop after that; needs no GPU) and `--write_colate_mat` (write
// <output>.colate_mat exactly as the reference does for BCF/BAM inputs, coal.cpp:3336-3343, 3453-3470).

const char* const kValueOptions[] = {
    "mode", "anc", "mut", "target_bcf", "reference_bcf", "target_mask", "reference_mask",
    "target_table", "target_bam", "reference_bam", "target_tmp", "reference_tmp", "target_age",
    "reference_age", "ref_genome", "anc_genome", "mask", "mask_cutoff", "chr", "bins",
    "lineage_bin", "outgroup_tmrca", "years_per_gen", "coal", "seed", "num_bootstraps", "filters",
    "groups", "poplabels", "map", "input", "output", "device", "devices", "ranks", "counts_out", "pairs",
    "rows", "max_iter", "min_iter", "write_rows", "samples", "age_profile"};
const char* const kBoolOptions[] = {"help", "strandfilter", "counts_only", "write_colate_mat", "profile_only"};

bool parse_options(int argc, char** argv, Options& o, std::string& err) {
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    std::string name, value;
    bool have_value = false;
    if (a.rfind("--", 0) == 0) {
      name = a.substr(2);
      size_t eq = name.find('=');
      if (eq != std::string::npos) {
        value = name.substr(eq + 1);
        name = name.substr(0, eq);
        have_value = true;
      }
    } else if (a == "-i") {
      name = "input";
    } else if (a == "-o") {
      name = "output";
    } else {
      err = "Unexpected argument '" + a + "'";
      return false;
    }
    if (name == "num_bootstrap") name = "num_bootstraps";
    bool is_bool = false, known = false;
    for (const char* b : kBoolOptions)
      if (name == b) is_bool = known = true;
    for (const char* v : kValueOptions)
      if (name == v) known = true;
    if (!known) {
      err = "Option '" + name + "' does not exist";
      return false;
    }
    if (is_bool) {
      o.kv[name] = "true";
      continue;
    }
    if (!have_value) {
      if (i + 1 >= argc) {
        err = "Option '" + name + "' is missing an argument";
        return false;
      }
      value = argv[++i];
    }
    o.kv[name] = value;
  }
  return true;
}

void print_help() {
  std::cout << "Usage:\n  Colate [OPTION...]\n\n"
            << "      --help                 Print help.\n"
            << "      --mode arg             Choose which part of the algorithm to run (colate_amd: mut, mut_interval, compare_tmp, count_topo, make_tmp, CondCoalRates).\n"
            << "      --mut arg              Filename of file containing mut.\n"
            << "      --target_tmp arg       Filename of target tmp file\n"
            << "      --reference_tmp arg    Filename of reference tmp file\n"
            << "      --target_mask arg      Fasta file containing target mask\n"
            << "      --reference_mask arg   Fasta file containing reference mask\n"
            << "      --target_age arg       Target age in years\n"
            << "      --reference_age arg    Reference age in years\n"
            << "      --chr arg              Optional: File specifying chromosomes to use.\n"
            << "      --bins arg             Optional: Epoch boundaries 10^(seq(x,y,stepsize)) [format: x,y,stepsize]. In years.\n"
            << "      --years_per_gen arg    Optional: Years per generation.\n"
            << "      --coal arg             Filename of file containing coalescence rates.\n"
            << "      --seed arg             Optional: Seed for random number generator (int)\n"
            << "      --num_bootstraps arg   Optional: Number of bootstraps.\n"
            << "      --device arg           Optional (colate_amd): GPU ordinal, default 0.\n"
            << "      --devices arg          Optional (colate_amd): shard the bootstrap replicates over GPUs 0..N-1 (one process).\n"
            << "      --ranks arg            Optional (colate_amd): the same as N processes, one per GPU, one RCCL all-gather.\n"
            << "      --pairs arg            Optional (colate_amd): file of `target_tmp reference_tmp output [target_age [reference_age]]`\n"
            << "                             lines; all pairs share --mut/--chr/--bins/--num_bootstraps/--seed, each .mut is parsed\n"
            << "                             once and all replicates of all pairs run in one GPU launch.  After the three names a\n"
            << "                             line may carry, in any order and mixed with the ages, target_mask=PREFIX,\n"
            << "                             reference_mask=PREFIX (expanded as --target_mask / --reference_mask are) and\n"
            << "                             coal=FILE (the pair's --coal warm start; --bins is then not needed for that line).\n"
            << "                             (--mode mut_interval) --pairs FILE with --mut [--chr, --bins]: the same lines without ages;\n"
            << "                             every pair's interval-dated fit in one pass, each <output>.coal that of its single run.\n"
            << "      --samples arg          (--mode mut_interval) file of `NAME FILE.colate.in [mask=PREFIX] [role=target|reference]`\n"
            << "                             lines; with --mut, -o PREFIX [--chr] and --bins or --coal every target x reference pair of\n"
            << "                             different lines is fitted, the pairs walked on the GPU; writes PREFIX_<target>_<reference>.coal,\n"
            << "                             each the file `--pairs` writes for that pair.\n"
            << "                             (--mode mut) the same list, a line may add age=YEARS; the pairs are walked and their tables\n"
            << "                             filled on the GPU; PREFIX_<target>_<reference>.coal (and .counts) as `--mode mut --pairs` writes them.\n"
            << "                             (--mode compare_tmp) the same list without mask= and age=; with --mut and -o PREFIX every pair's\n"
            << "                             windowed mismatch counts, compared on the GPU: PREFIX_<target>_<reference>.txt and PREFIX.pairs.txt.\n"
            << "                             (--mode count_topo) that list with role= a comma-separated subset of cond,target,reference (default: all\n"
            << "                             three); every (cond, target, reference) of three lines, drawn on the GPU: PREFIX_<cond>_<target>_<reference>.txt\n"
            << "                             and PREFIX.triples.txt.\n"
            << "      --age_profile arg      (--mode count_topo --samples) x,y,stepsize as for --bins [--years_per_gen, default 28]: also write\n"
            << "                             PREFIX.profile.txt, `cond target reference epoch plus minus qualifying` per (triple, epoch): the\n"
            << "                             printed rows of either sign and the rows that drew, binned on the GPU by the mid of their ages.\n"
            << "      --profile_only         (--mode count_topo --samples --age_profile) write no per-triple file: PREFIX.profile.txt and\n"
            << "                             PREFIX.triples.txt only.\n"
            << "      --counts_out arg       Optional (colate_amd): write the bootstrap count tables (.colate_mat layout).\n"
            << "      --counts_only          Optional (colate_amd): stop after --counts_out (no GPU needed).\n"
            << "      --write_colate_mat     Optional (colate_amd): write <output>.colate_mat as the reference does for BCF/BAM inputs.\n"
            << "      --target_table arg     (--mode make_tmp) Table `chr bp allele` of the target's calls.\n"
            << "      --ref_genome arg       (--mode make_tmp) Reference genome fasta (per chromosome with --chr).\n"
            << "      --input arg            (--mode CondCoalRates) Prefix of the Relate .anc / .mut files.\n"
            << "      --poplabels arg        (--mode CondCoalRates) Poplabels file (groups: its second column).\n"
            << "      --groups arg           (--mode CondCoalRates) FOCAL,CONDITIONAL group names.\n"
            << "      --lineage_bin arg      (--mode CondCoalRates) log10 of the focal epoch boundary in years (default 1e5).\n"
            << "      --mask arg             (--mode CondCoalRates) Fasta mask (per chromosome with --chr).\n"
            << "                             (--mode CondCoalRates) --pairs FILE: `FOCAL,CONDITIONAL OUTPUT` per line, in place of\n"
            << "                             --groups / --output; every table is its single run's, from one pass over the trees.\n"
            << "      --rows arg             (--mode mut_interval) File of `block kind age_begin age_end weight` lines (plain or gzip):\n"
            << "                             block a non-negative integer, kind shared|notshared, ages in generations; with --bins or\n"
            << "                             --coal, --num_bootstraps, --seed, --years_per_gen; writes <output>.coal.\n"
            << "                             (--mode mut_interval) or --mut, --target_tmp, --reference_tmp [--chr, --target_mask,\n"
            << "                             --reference_mask] as for --mode mut: every used SNP is one interval-dated observation.\n"
            << "      --write_rows arg       (--mode mut_interval) Write the rows and per-block weights in the --rows format.\n"
            << "      --max_iter arg         (--mode mut_interval) Iteration cap of the EM (default 100000).\n"
            << "      --min_iter arg         (--mode mut_interval) Iterations before the stop rule applies (default 1000).\n"
            << "  -o, --output arg           Filename of output.\n"
            << std::endl;
}

// ------------------------------------------------------------------ stage timing (COLATE_TIMING=1: one stderr line at the end)
StageTimes g_times;

// ------------------------------------------------------------------ .mut rows

// (the readers run on their own threads: leave without running the static destructors under the other threads' feet)
[[noreturn]] void reader_exit() {
  std::cerr.flush();
  std::cout.flush();
  std::fflush(nullptr);
  std::_Exit(1);
}
[[noreturn]] void mut_line_error(const std::string& line) {
  std::cerr << "Error reading following line in mut file:" << std::endl;
  std::cerr << line << std::endl;
  reader_exit();
}

// std::stoi on the text at p (leading white space, sign, digits; what follows the digits is ignored), without the copy
// and the exceptions: false where std::stoi would throw (no digits, or out of int range)
inline bool parse_stoi(const char* p, const char* end, int& out, const char** after = nullptr) {
  while (p < end && (*p == ' ' || (*p >= '\t' && *p <= '\r'))) p++;
  bool neg = false;
  if (p < end && (*p == '+' || *p == '-')) neg = (*p++ == '-');
  if (p >= end || *p < '0' || *p > '9') return false;
  long long v = 0;
  while (p < end && *p >= '0' && *p <= '9') {
    v = v * 10 + (*p++ - '0');
    if (v > 2147483648LL) return false;
  }
  if (neg) v = -v;
  if (v > 2147483647LL || v < -2147483648LL) return false;
  out = (int)v;
  if (after) *after = p;
  return true;
}
// std::stof: strtof (the field ends at a ';' or at the terminating NUL of the line buffer, where strtof stops by itself)
inline bool parse_stof(const char* p, float& out) {
  char* e = nullptr;
  errno = 0;
  const float v = std::strtof(p, &e);
  if (e == p || errno == ERANGE) return false;
  out = v;
  return true;
}

// One row from the NUL-terminated line [b, e): the fields parse_tmptmp looks at (mutations.cpp:77-246)
inline bool parse_mut_line(char* b, char* e, MutRow& r) {
  // the first ten ';' of the line (snp;pos;dist;rs;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;<rest>)
  char* sep[11];
  int ns = 0;
  for (char* q = b; q < e && ns < 11; q++)
    if (*q == ';') sep[ns++] = q;
  if (ns < 10) return false;  // needs 10 separators
  int tmp;
  if (!parse_stoi(b, sep[0], tmp)) return false;
  if (!parse_stoi(sep[0] + 1, sep[1], r.pos)) return false;
  if (!parse_stoi(sep[1] + 1, sep[2], r.dist)) return false;
  if (!parse_stoi(sep[3] + 1, sep[4], r.tree)) return false;
  r.num_branches = 0;
  for (const char* q = sep[4] + 1; q < sep[5];) {  // white-space separated branch indices, each through stoi
    while (q < sep[5] && (*q == ' ' || (*q >= '\t' && *q <= '\r'))) q++;
    if (q >= sep[5]) break;
    const char* tok_end = q;
    while (tok_end < sep[5] && !(*tok_end == ' ' || (*tok_end >= '\t' && *tok_end <= '\r'))) tok_end++;
    if (!parse_stoi(q, tok_end, tmp)) return false;
    r.num_branches++;
    q = tok_end;
  }
  if (!parse_stoi(sep[6] + 1, sep[7], r.flipped)) return false;
  *sep[8] = 0;  // (strtof must not read past its field: "1e5;2" is fine, but keep it strict)
  const bool ok1 = parse_stof(sep[7] + 1, r.age_begin);
  *sep[8] = ';';
  *sep[9] = 0;
  const bool ok2 = parse_stof(sep[8] + 1, r.age_end);
  *sep[9] = ';';
  if (!ok1 || !ok2) return false;
  // field 10: up to the next ';' or the end of the line; "NA" is kept when it is empty and the last field
  char* f10_end = (ns >= 11) ? sep[10] : e;
  if (f10_end > sep[9] + 1 || ns >= 11)
    r.mutation_type.assign(sep[9] + 1, f10_end);
  else
    r.mutation_type = "NA";
  return true;
}

bool for_each_mut_row(const std::string& filename, const std::function<void(const MutRow&)>& sink) {
  gzFile f = gzopen(filename.c_str(), "rb");
  if (!f) f = gzopen((filename + ".gz").c_str(), "rb");
  if (!f) {
    std::cerr << "Error while reading " << filename << "(.gz)." << std::endl;
    reader_exit();  // mutations.cpp:265-268: exit(1)
  }
  gzbuffer(f, 1 << 20);
  MutRow row;
  // inflate in 4 MB pieces and cut lines in place (no per-line std::string, no per-field copies)
  std::vector<char> buf((4u << 20) + 1);
  size_t have = 0;
  bool header_done = false, eof = false;
  while (!eof) {
    if (have == buf.size() - 1) buf.resize(buf.size() * 2);  // a line longer than the buffer
    const int got = gzread(f, buf.data() + have, (unsigned)(buf.size() - 1 - have));
    if (got <= 0) eof = true;
    else have += (size_t)got;
    char* b = buf.data();
    char* const end = b + have;
    for (;;) {
      char* nl = static_cast<char*>(std::memchr(b, '\n', (size_t)(end - b)));
      if (!nl) {
        if (!eof || b == end) break;
        nl = end;  // last line without a newline
      }
      *nl = 0;
      if (!header_done) {
        header_done = true;
      } else {
        row.mutation_type = "NA";
        if (!parse_mut_line(b, nl, row)) mut_line_error(std::string(b, nl));
        sink(row);
      }
      b = (nl < end) ? nl + 1 : end;
      if (b >= end) break;
    }
    have = (size_t)(end - b);
    if (have) std::memmove(buf.data(), b, have);
  }
  gzclose(f);
  return true;
}

bool read_mut_file(const std::string& filename, std::vector<MutRow>& rows) {
  rows.clear();
  return for_each_mut_row(filename, [&rows](const MutRow& r) { rows.push_back(r); });
}

// data.cpp:213-235: sequence = upper-cased lines after the header, concatenated (also read on the engine's pool threads)
static void open_fasta_mask(GzText& is, const std::string& filename) {
  if (!is.open(filename) && !is.open(filename + ".gz")) {
    std::cerr << "Error while opening file " << filename << "." << std::endl;
    reader_exit();  // (data.cpp: exit(1))
  }
}

void check_fasta_mask(const std::string& filename) {
  GzText is;
  open_fasta_mask(is, filename);
}

void read_fasta_mask(const std::string& filename, std::string& seq) {
  GzText is;
  open_fasta_mask(is, filename);
  std::string line;
  is.getline(line);
  seq.clear();
  while (is.getline(line)) {
    for (char& c : line) c = (char)std::toupper((unsigned char)c);
    seq += line;
  }
}

// ------------------------------------------------------------------ .colate.in
// Record (little-endian, no header), coal.cpp:2505-2514 / 2126-2133:
//   int32 lchrom; char chrom[lchrom]; int32 bp; char anc; char der; int32 AAF; int32 DAF
struct TmpStream {
  FILE* fp = nullptr;
  std::string chrom;  // name of the record last read ("" before any read)
  int bp = 0;
  char anc = 0, der = 0;
  int AAF = 0, DAF = 0;  // the reference resets these two between SNPs (coal.cpp:2182-2183)
  // returns false at end of file, leaving every field as it was (coal.cpp:2126 `break`).  The seven fread calls of the
  // reference per record, served from a buffer of our own (40 M records x 7 library calls were 3 s of the table fill); a
  // field cut short by the end of the file keeps the bytes that were there, as with fread.
  bool next() {
    int lchrom = 0;
    if (!fp || get(&lchrom, sizeof(int)) != sizeof(int)) return false;
    char buf[1024];
    if (lchrom < 0 || lchrom > 1023) lchrom = 0;
    get(buf, (size_t)lchrom);
    chrom.assign(buf, (size_t)lchrom);
    get(&bp, sizeof(int));
    get(&anc, 1);
    get(&der, 1);
    get(&AAF, sizeof(int));
    get(&DAF, sizeof(int));
    return true;
  }

 private:
  size_t get(void* dst, size_t n) {
    if (end_ - pos_ < n) refill();
    const size_t k = std::min(n, end_ - pos_);
    std::memcpy(dst, buf_.data() + pos_, k);
    pos_ += k;
    return k;
  }
  void refill() {
    if (buf_.empty()) buf_.resize(1u << 20);
    const size_t keep = end_ - pos_;
    if (keep) std::memmove(buf_.data(), buf_.data() + pos_, keep);
    pos_ = 0, end_ = keep;
    if (!eof_) {
      const size_t got = std::fread(buf_.data() + end_, 1, buf_.size() - end_, fp);
      end_ += got;
      if (got == 0) eof_ = true;
    }
  }
  std::vector<char> buf_;
  size_t pos_ = 0, end_ = 0;
  bool eof_ = false;
};



// coal.cpp:2071-2321, on the calling thread.  Returns the number of blocks.
int fill_tables_from_tmp(const std::vector<std::string>& chr_names,
                         const std::vector<std::string>& mut_files, const std::string& target_file,
                         const std::string& ref_file, const std::vector<std::string>& target_masks,
                         const std::vector<std::string>& ref_masks, double C, std::mt19937& rng,
                         int num_bases_per_block, int A, PairTables& tab) {
  const double age = 0, ref_age = 0;  // forced, coal.cpp:2074-2075
  std::uniform_real_distribution<double> dist_unif(0, 1);
  const float num_samples = 100;
  TmpStream tgt, ref;
  tgt.fp = std::fopen(target_file.c_str(), "rb");
  ref.fp = std::fopen(ref_file.c_str(), "rb");
  if (!tgt.fp) std::cerr << "Failed to open " << target_file << std::endl;
  if (!ref.fp) std::cerr << "Failed to open " << ref_file << std::endl;
  const bool has_tar_mask = !target_masks.empty(), has_ref_mask = !ref_masks.empty();

  // [nb][A] tables, one block of A zeros per genome block (the block being filled is the last)
  int num_blocks = 0;
  size_t blk = 0;
  for (std::vector<double>* t : {&tab.sh, &tab.ns, &tab.she, &tab.nse}) t->assign((size_t)A, 0.0);
  auto advance_block = [&]() {
    blk++;
    num_blocks++;
    for (std::vector<double>* t : {&tab.sh, &tab.ns, &tab.she, &tab.nse}) t->resize((blk + 1) * A, 0.0);
  };

  std::vector<MutRow> rows;
  std::string tar_mask, ref_mask;
  for (size_t chr = 0; chr < mut_files.size(); chr++) {
    std::cerr << "parsing CHR: " << chr + 1 << " / " << mut_files.size() << std::endl;
    const double t_parse0 = StageTimes::now();
    read_mut_file(mut_files[chr], rows);
    const double t_fill0 = StageTimes::now();
    g_times.parse_mut += t_fill0 - t_parse0;
    if (has_tar_mask) read_fasta_mask(target_masks[chr], tar_mask);
    if (has_ref_mask) read_fasta_mask(ref_masks[chr], ref_mask);
    int current_block_base = 0;
    const std::string& name = chr_names[chr];
    while (ref.chrom != name) {  // skip to this chromosome, coal.cpp:2125-2134
      if (!ref.next()) break;
    }
    while (tgt.chrom != name) {
      if (!tgt.next()) break;
    }
    for (const MutRow& m : rows) {
      if (!(m.flipped == 0 && m.num_branches == 1 && m.age_begin < m.age_end && m.age_end >= age))
        continue;
      // "anc/der" (mutations.cpp:236-246 splits at the first '/'): both sides as views into the row's string
      const std::string& mt = m.mutation_type;
      const size_t slash = mt.find('/');
      const size_t anc_len = slash == std::string::npos ? mt.size() : slash;
      const char* const anc_p = mt.data();
      const char* const der_p = slash == std::string::npos ? mt.data() + mt.size() : mt.data() + slash + 1;
      const size_t der_len = slash == std::string::npos ? 0 : mt.size() - slash - 1;
      const int bp_mut = m.pos;
      if (anc_len == 0 || der_len == 0) continue;
      const char anc0 = anc_p[0], der0 = der_p[0];

      bool use = true;
      if (has_tar_mask && (size_t)bp_mut < tar_mask.size() && tar_mask[bp_mut - 1] != 'P') use = false;
      if (has_ref_mask && (size_t)bp_mut < ref_mask.size() && ref_mask[bp_mut - 1] != 'P') use = false;
      if (!(anc_len == 1 && (anc0 == 'A' || anc0 == 'C' || anc0 == 'G' || anc0 == 'T' || anc0 == '0'))) use = false;
      if (!(der_len == 1 && (der0 == 'A' || der0 == 'C' || der0 == 'G' || der0 == 'T' || der0 == '1'))) use = false;

      if (use) {  // reference sample must carry the derived allele, coal.cpp:2181-2199
        ref.DAF = 0;
        ref.AAF = 0;
        while (ref.chrom == name && ref.bp < bp_mut) {
          if (!ref.next()) break;
        }
        if (ref.chrom != name || ref.bp != bp_mut || ref.anc != anc0 || ref.der != der0) use = false;
      }
      if (ref.DAF == 0) use = false;
      const int N_ref = ref.DAF + ref.AAF;

      if (use) {  // coal.cpp:2201-2219
        tgt.DAF = 0;
        tgt.AAF = 0;
        while (tgt.chrom == name && tgt.bp < bp_mut) {
          if (!tgt.next()) break;
        }
        if (tgt.chrom != name || tgt.bp != bp_mut || tgt.anc != anc0 || tgt.der != der0) use = false;
      }
      const int N_target = tgt.DAF + tgt.AAF;
      if (N_target == 0) use = false;
      if (!use) continue;

      double age_begin = m.age_begin;
      if (age_begin < ref_age) age_begin = ref_age;
      while (current_block_base + num_bases_per_block < bp_mut) {  // coal.cpp:2227-2234
        current_block_base += num_bases_per_block;
        advance_block();
      }
      // target genotype rounded to a diploid call, in float (coal.cpp:2236-2242)
      float f_DAF_target = tgt.DAF, f_AAF_target = tgt.AAF;
      f_DAF_target /= N_target / 2.0;
      f_AAF_target /= N_target / 2.0;
      f_DAF_target = std::round(f_DAF_target);
      f_AAF_target = std::round(f_AAF_target);

      double* const sh = tab.sh.data() + blk * A;
      double* const ns = tab.ns.data() + blk * A;
      const int DAF_ref = ref.DAF;
      if (age_begin <= age) {  // coal.cpp:2245-2275
        const int bin2 = age_bin_index(m.age_end, C);
        if (bin2 < A) {  // row 0 of the A*A table; larger indices land in rows nobody reads
          tab.she[blk * A + bin2] += f_DAF_target * DAF_ref / ((double)N_ref);
          tab.nse[blk * A + bin2] += f_AAF_target * DAF_ref / ((double)N_ref);
        }
        for (int j = 0; j < num_samples; j++) {
          double sampled_age = dist_unif(rng) * (m.age_end - age_begin) + age_begin;
          if (sampled_age < age) sampled_age = age;
          const int bin = age_bin_index(sampled_age, C);
          if (bin < A) ns[bin] += f_AAF_target * DAF_ref / ((double)N_ref * num_samples);
        }
      } else {  // coal.cpp:2277-2297
        int j = 0;
        while (j < num_samples) {
          const double sampled_age = dist_unif(rng) * (m.age_end - age_begin) + age_begin;
          bool skip = sampled_age < age;
          const int bin = age_bin_index(sampled_age, C);
          if (bin >= A) skip = true;
          if (!skip) {
            sh[bin] += f_DAF_target * DAF_ref / ((double)N_ref * num_samples);
            ns[bin] += f_AAF_target * DAF_ref / ((double)N_ref * num_samples);
            j++;
          }
        }
      }
    }
    advance_block();  // chromosome end, coal.cpp:2306-2310
    g_times.table_fill += StageTimes::now() - t_fill0;
  }
  if (tgt.fp) std::fclose(tgt.fp);
  if (ref.fp) std::fclose(ref.fp);
  for (std::vector<double>* t : {&tab.sh, &tab.ns, &tab.she, &tab.nse}) t->resize((size_t)num_blocks * A);
  tab.nb = num_blocks;
  return num_blocks;
}


// OUT.colate_mat (coal.cpp:3471-3499): 185 grid values, then per replicate 185 shared
// and 185 not-shared counts, read with operator>> (a failed extraction leaves zeros).
bool load_colate_mat(const std::string& path, int B, int A, std::vector<double>& grid,
                     std::vector<double>& csh, std::vector<double>& cns) {
  GzText is;
  if (!is.open(path)) return false;
  std::string all, line;
  while (is.getline(line)) {
    all += line;
    all += '\n';
  }
  std::istringstream ss(all);
  for (int b = 0; b < A; b++) ss >> grid[b];
  csh.assign((size_t)B * A, 0.0);
  cns.assign((size_t)B * A, 0.0);
  for (int i = 0; i < B; i++) {
    for (int b = 0; b < A; b++) ss >> csh[(size_t)i * A + b];
    for (int b = 0; b < A; b++) ss >> cns[(size_t)i * A + b];
  }
  return true;
}

bool file_exists(const std::string& p) {
  FILE* f = std::fopen(p.c_str(), "rb");
  if (!f) return false;
  std::fclose(f);
  return true;
}

RankCtx g_rank;

bool write_all(int fd, const void* buf, size_t n) {
  const char* p = static_cast<const char*>(buf);
  while (n) {
    ssize_t k = ::write(fd, p, n);
    if (k <= 0) return false;
    p += k, n -= (size_t)k;
  }
  return true;
}
bool read_all(int fd, void* buf, size_t n) {
  char* p = static_cast<char*>(buf);
  while (n) {
    ssize_t k = ::read(fd, p, n);
    if (k <= 0) return false;
    p += k, n -= (size_t)k;
  }
  return true;
}

void print_usage_footer() {  // coal.cpp:3852-3861
  rusage usage;
  getrusage(RUSAGE_SELF, &usage);
  std::cerr << "CPU Time spent: " << usage.ru_utime.tv_sec << "." << std::setfill('0') << std::setw(6)
            << usage.ru_utime.tv_usec << "s; Max Memory usage: " << usage.ru_maxrss / 1000.0 << "Mb." << std::endl;
  std::cerr << "---------------------------------------------------------" << std::endl << std::endl;
}

// coal.cpp:3295-3313: with --chr one .mut (<mut>_chr<name>.mut) and one fasta per mask (<mask>_chr<name>.fa) per listed
// chromosome, else the paths verbatim and the chromosome name ""
void chromosome_files(const Options& opt, std::vector<std::string>& names, std::vector<std::string>& mut_files,
                      std::vector<std::string>* target_masks, std::vector<std::string>* ref_masks) {
  if (opt.has("chr")) {
    GzText is_chr;
    if (!is_chr.open(opt.get("chr"))) std::cerr << "Error while opening file " << opt.get("chr") << std::endl;
    std::string line;
    while (is_chr.getline(line)) {
      names.push_back(line);
      mut_files.push_back(opt.get("mut") + "_chr" + line + ".mut");
    }
  } else {
    names.push_back("");
    mut_files.push_back(opt.get("mut"));
  }
  if (target_masks && opt.has("target_mask")) *target_masks = mask_files(opt, names, opt.get("target_mask"));
  if (ref_masks && opt.has("reference_mask")) *ref_masks = mask_files(opt, names, opt.get("reference_mask"));
}

std::vector<std::string> mask_files(const Options& opt, const std::vector<std::string>& names, const std::string& prefix) {
  if (!opt.has("chr")) return {prefix};
  std::vector<std::string> files;
  for (const std::string& n : names) files.push_back(prefix + "_chr" + n + ".fa");
  return files;
}

// ------------------------------------------------------------------ what the single-pair and the --pairs drivers share
// (mut_feeder.h)
int api_error(int rc) {
  std::cerr << "Error: " << colate_last_error() << " (" << rc << ")" << std::endl;
  return 1;
}

namespace {

// The settings every pair of a run shares: --years_per_gen, the age grid of the A bins, then (read_replicates) the seed of
// the run's generator and the number of bootstrap replicates B.  Two steps: the single-pair driver prints its sample age
// and the number of bins in between.
struct RunSetup {
  double years_per_gen = 28.0;
  std::vector<double> age_grid;
  int A = 0, seed = 0, B = 1;
  explicit RunSetup(const Options& opt) : age_grid(256) {
    if (opt.has("years_per_gen")) years_per_gen = std::stof(opt.get("years_per_gen"));
    A = colate_age_grid(age_grid.data(), 256);
    age_grid.resize(A);
  }
  bool read_replicates(const Options& opt) {  // false after the error message
    seed = std::time(0) + getpid();  // coal.cpp:3158
    if (opt.has("seed")) seed = std::stoi(opt.get("seed"));
    if (opt.has("num_bootstraps")) B = std::stoi(opt.get("num_bootstraps"));
    if (B < 1) {
      std::cerr << "Error: --num_bootstraps must be at least 1." << std::endl;
      return false;
    }
    return true;
  }
};

// One process, one GPU: create the HIP context on a second thread while this one reads the inputs (a fresh process pays a
// few hundred ms for it; end to end 0.63 -> see profiles/r02/bench/e2e.txt); joined when the guard goes.  Not with --ranks
// (every rank picks its own device after the fork) or --devices (several contexts), not when no device is needed.
struct DeviceWarmUp {
  std::thread t;
  explicit DeviceWarmUp(const Options& opt) {
    if (g_rank.ranked || opt.has("devices") || opt.has("counts_only")) return;
    int dev = 0;  // the device the run will use (--device N)
    try {
      if (opt.has("device")) dev = std::stoi(opt.get("device"));
    } catch (...) {
      dev = 0;  // (reported where the option is used)
    }
    t = std::thread([dev] { (void)colate_warm_up(dev); });
  }
  ~DeviceWarmUp() {
    if (t.joinable()) t.join();
  }
};

// A pair's epochs and starting rates (coal.cpp:3501-3646): from the .coal file `coal` (which gives the rates too; ep_null 0)
// or, without one, from --bins and the pair's age.  Returns E, the two vectors sized to it, or <= 0 (colate_last_error()).
int pair_epochs(const Options& opt, const std::string* coal, double age, double years_per_gen, std::vector<double>& epochs,
                std::vector<double>& init, int& ep_null) {
  epochs.assign(COLATE_MAX_EPOCHS, 0.0);
  init.assign(COLATE_MAX_EPOCHS, COLATE_DEFAULT_INIT_RATE);
  ep_null = 0;
  const int E = coal ? colate_epochs_from_coal(coal->c_str(), age, epochs.data(), init.data(), COLATE_MAX_EPOCHS)
                     : colate_epochs_from_bins(opt.get("bins").c_str(), age, years_per_gen, epochs.data(), COLATE_MAX_EPOCHS, &ep_null);
  if (E > 0) epochs.resize(E), init.resize(E);
  return E;
}

// --device N: this process's GPU (a rank picks its own, RankComm); --devices N: `devs` = 0..N-1 to shard the rows over
// (left empty without it).  False after the error message.
bool bind_devices(const Options& opt, std::vector<int>& devs) {
  if (opt.has("device") && !g_rank.ranked) {
    if (int rc = colate_set_device(std::stoi(opt.get("device")))) {
      api_error(rc);
      return false;
    }
  }
  if (opt.has("devices")) {
    const int nd = std::stoi(opt.get("devices"));
    if (nd < 1) {
      std::cerr << "Error: --devices must be at least 1." << std::endl;
      return false;
    }
    for (int d = 0; d < nd; d++) devs.push_back(d);
  }
  return true;
}

// `--ranks`: this rank's GPU, (--device + rank) % the node's devices, and the RCCL communicator of all ranks, whose id rank 0
// creates and the launcher relays (run_ranked).  The communicator is destroyed with the object.
struct RankComm {
  void* comm = nullptr;
  RankComm() = default;
  RankComm(const RankComm&) = delete;
  RankComm& operator=(const RankComm&) = delete;
  ~RankComm() { colate_comm_destroy(comm); }

  bool open(const Options& opt) {  // false after the error message
#ifdef COLATE_TEST_HOOKS  // (only in lib/testhooks/libcolate_amd.so, which the tests of the launcher load: never in the product library)
    if (const char* h = std::getenv("COLATE_TEST_HANG_RANK")) {  // a rank stuck as if inside a collective
      if (std::atoi(h) == g_rank.rank)
        for (;;) ::pause();
    }
#endif
    const int ndev = colate_device_count();
    if (ndev < 1) {
      std::cerr << "Error: " << colate_last_error() << std::endl;
      return false;
    }
    const int dev0 = opt.has("device") ? std::stoi(opt.get("device")) : 0;
    unsigned char id[COLATE_COMM_ID_BYTES];
    int rc = colate_set_device((dev0 + g_rank.rank) % ndev);
    if (!rc) {
      if (g_rank.rank == 0) {
        rc = colate_comm_unique_id(id);
        if (!write_all(g_rank.fd_id_out, id, rc ? 0 : sizeof(id)) && !rc) rc = COLATE_EIO;
        ::close(g_rank.fd_id_out);  // (on failure the launcher sees end-of-file and tells the others)
      } else if (!read_all(g_rank.fd_id_in, id, sizeof(id))) {
        std::cerr << "Error: rank " << g_rank.rank << " did not receive the communicator id." << std::endl;
        return false;
      }
    }
    if (!rc) rc = colate_comm_create(id, g_rank.nranks, g_rank.rank, &comm);
    if (rc) api_error(rc);
    return !rc;
  }
};

// The lines of one pair's B replicates.  `pair`: the pair's number in a --pairs list, which then leads each line; 0 for the
// single pair.
void report_replicates(int pair, int B, int E, const int* iters, const int* flags) {
  const std::string p = std::to_string(pair);
  int unresolved_max = 0;
  for (int i = 0; i < B; i++) {
    std::cerr << (pair ? "Pair " + p + " " : "") << "Bootstrap " << i + 1 << ": Total iterations " << iters[i] << std::endl;
    if (flags[i] & (COLATE_FLAG_NAN | COLATE_FLAG_NEG))
      std::cerr << "Warning: " << (pair ? "pair " + p + " " : "") << "bootstrap " << i + 1
                << " produced NaN or negative sufficient statistics (the reference aborts here)." << std::endl;
    unresolved_max = std::max(unresolved_max, COLATE_UNRESOLVED_EPOCHS(flags[i]));
  }
  if (unresolved_max > 0)  // (include/colate_amd.h, COLATE_FLAG_UNRESOLVED)
    std::cerr << "Note: " << (pair ? "pair " + p + ": " : "") << "the last " << unresolved_max << " of " << E
              << " epochs are older than the data resolve: "
              << "their printed rates depend on rounding residue (in the reference build too) and are not reproducible."
              << std::endl;
}

}  // namespace

// (mut_feeder.h)
bool read_pair_list(const std::string& path, const Options& opt, const std::vector<std::string>& chr_names, std::vector<PairSpec>& pairs) {
  std::ifstream is(path);
  if (!is) {
    std::cerr << "Error while opening file " << path << std::endl;
    return false;
  }
  std::string line;
  for (size_t line_no = 1; std::getline(is, line); line_no++) {
    std::istringstream ss(line);
    PairSpec ps;
    if (!(ss >> ps.target >> ps.reference >> ps.output)) continue;
    auto fail = [&](const std::string& what) {
      std::cerr << "Error: " << path << ", line " << line_no << ": " << what << std::endl;
      return false;
    };
    int n_ages = 0;
    bool seen_tm = false, seen_rm = false, seen_coal = false;
    for (std::string tok; ss >> tok;) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        if (n_ages == 2) return fail("more than two ages ('" + tok + "')");
        float v = 0;
        size_t used = 0;
        try {
          v = std::stof(tok, &used);
        } catch (...) {
          used = 0;
        }
        if (used == 0 || used != tok.size()) return fail("the age '" + tok + "' is not a number");
        (n_ages++ == 0 ? ps.target_age : ps.ref_age) = v;
        continue;
      }
      const std::string key = tok.substr(0, eq), value = tok.substr(eq + 1);
      bool* seen = key == "target_mask" ? &seen_tm : key == "reference_mask" ? &seen_rm : key == "coal" ? &seen_coal : nullptr;
      if (!seen) return fail("unknown key '" + key + "' (known: target_mask, reference_mask, coal)");
      if (*seen) return fail("the key '" + key + "' is given twice");
      if (value.empty()) return fail("the key '" + key + "' has no value");
      *seen = true;
      if (key == "target_mask") ps.target_masks = mask_files(opt, chr_names, value);
      else if (key == "reference_mask") ps.ref_masks = mask_files(opt, chr_names, value);
      else ps.coal = value;
    }
    ps.line = line_no, ps.ages_given = n_ages;
    pairs.push_back(ps);
  }
  if (pairs.empty()) {
    std::cerr << "Error: no pairs in " << path << std::endl;
    return false;
  }
  return true;
}

// (mut_feeder.h)
bool read_sample_list(const std::string& path, const Options& opt, const std::vector<std::string>& chr_names, bool with_ages,
                      std::vector<SampleLine>& samples, bool with_cond) {
  std::ifstream is(path);
  if (!is) {
    std::cerr << "Error while opening file " << path << std::endl;
    return false;
  }
  std::string line;
  for (size_t line_no = 1; std::getline(is, line); line_no++) {
    auto fail = [&](const std::string& what) {
      std::cerr << "Error: " << path << ", line " << line_no << ": " << what << std::endl;
      return false;
    };
    std::istringstream ss(line);
    SampleLine sl;
    sl.line = line_no, sl.cond = with_cond;
    if (!(ss >> sl.name)) continue;  // a blank line
    if (sl.name.find('=') != std::string::npos) return fail("the line starts with '" + sl.name + "': the sample's NAME is missing or empty");
    if (sl.name.find('/') != std::string::npos) return fail("the NAME '" + sl.name + "' contains '/'");
    if (!(ss >> sl.file) || sl.file.find('=') != std::string::npos)
      return fail(with_ages ? "expected `NAME FILE.colate.in [mask=PREFIX] [role=target|reference] [age=YEARS]`"
                            : "expected `NAME FILE.colate.in [mask=PREFIX] [role=target|reference]`");
    for (const SampleLine& other : samples)
      if (other.name == sl.name) return fail("the NAME '" + sl.name + "' is given twice (first on line " + std::to_string(other.line) + ")");
    bool seen_mask = false, seen_role = false, seen_age = false;
    for (std::string tok; ss >> tok;) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos)
        return fail("'" + tok + "' is no key=value token (" +
                    (with_ages ? "a sample's age is given as age=YEARS)" : "--mode mut_interval takes modern samples only: a line cannot carry sample ages)"));
      const std::string key = tok.substr(0, eq), value = tok.substr(eq + 1);
      bool* seen = key == "mask" ? &seen_mask : key == "role" ? &seen_role : (with_ages && key == "age") ? &seen_age : nullptr;
      if (!seen) return fail("unknown key '" + key + (with_ages ? "' (known: mask, role, age)" : "' (known: mask, role)"));
      if (*seen) return fail("the key '" + key + "' is given twice");
      if (value.empty()) return fail("the key '" + key + "' has no value");
      *seen = true;
      if (key == "mask") sl.masks = mask_files(opt, chr_names, value);
      else if (key == "age") {  // (read as the ages of a `--pairs` line are)
        float v = 0;
        size_t used = 0;
        try {
          v = std::stof(value, &used);
        } catch (...) {
          used = 0;
        }
        if (used == 0 || used != value.size() || !(v == v)) return fail("the age '" + value + "' is not a number");
        if (v < 0) return fail("the age '" + value + "' is negative");
        sl.age = v;
      } else if (with_cond) {  // (`--mode count_topo`: a comma-separated subset of the three roles)
        sl.cond = sl.target = sl.reference = false;
        std::istringstream roles(value);
        for (std::string r; std::getline(roles, r, ',');) {
          bool* const on = r == "cond" ? &sl.cond : r == "target" ? &sl.target : r == "reference" ? &sl.reference : nullptr;
          if (!on) return fail("unknown role '" + r + "' (known: cond, target, reference)");
          if (*on) return fail("the role '" + r + "' is given twice");
          *on = true;
        }
      } else if (value == "target") sl.reference = false;
      else if (value == "reference") sl.target = false;
      else return fail("unknown role '" + value + "' (known: target, reference)");
    }
    samples.push_back(sl);
  }
  bool any_t = false, any_r = false, any_c = !with_cond;
  for (const SampleLine& sl : samples) any_t = any_t || sl.target, any_r = any_r || sl.reference, any_c = any_c || sl.cond;
  if (!any_c) {
    std::cerr << "Error: " << path << ": the list names no cond sample." << std::endl;
    return false;
  }
  if (!any_t || !any_r) {
    std::cerr << "Error: " << path << ": the list names no " << (!any_t ? "target" : "reference") << " sample." << std::endl;
    return false;
  }
  return true;
}

int run_mut(const Options& opt) {
  if (!opt.has("mut") || !opt.has("output")) {  // coal.cpp:3077-3087
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: mut, bins, output. Optional: target_tmp, reference_tmp, target_age, "
                 "reference_age, target_mask, reference_mask, coal, num_bootstrap."
              << std::endl;
    print_help();
    return 0;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates for (ancient) samples.." << std::endl;
  const DeviceWarmUp warm(opt);

  double target_age = 0, ref_age = 0;
  try {
    if (opt.has("target_age")) target_age = std::stof(opt.get("target_age"));
    if (opt.has("reference_age")) ref_age = std::stof(opt.get("reference_age"));
  } catch (...) {
    std::cerr << "Error: sample ages must be numbers." << std::endl;
    return 1;
  }
  if (!(target_age >= 0.0) || !(ref_age >= 0.0)) {
    std::cerr << "Error: sample ages must be non-negative." << std::endl;
    return 1;
  }
  RunSetup run(opt);
  const double age = std::max(target_age, ref_age) / run.years_per_gen;
  std::cerr << age << std::endl;
  const bool is_ancient = age > 0.0;

  const double C = 10;
  const int A = run.A;
  std::vector<double>& age_grid = run.age_grid;
  std::cerr << "num_bins: " << A << std::endl;
  if (!run.read_replicates(opt)) return 1;
  const int num_bases_per_block = 30e6, seed = run.seed, B = run.B;
  std::mt19937 rng(seed);
  const std::string out = opt.get("output");

  std::vector<double> csh, cns, weights;
  PairTables tab;  // (block bootstrap + F redistribution, coal.cpp:3326-3451, on its flat [nb][A] tables)
  int num_blocks = 0;
  bool gpu_bootstrap = false;
  const std::string mat = out + ".colate_mat";
  if (file_exists(mat)) {  // coal.cpp:3169-3170, 3471-3499
    std::cerr << "Loading precomputed file " << mat << std::endl;
    load_colate_mat(mat, B, A, age_grid, csh, cns);
  } else if (opt.has("target_tmp") && opt.has("reference_tmp")) {
    std::vector<std::string> names, mut_files;
    std::vector<PairSpec> one(1);
    PairSpec& pair = one[0];
    pair.target = opt.get("target_tmp"), pair.reference = opt.get("reference_tmp");
    chromosome_files(opt, names, mut_files, &pair.target_masks, &pair.ref_masks);
    // The pair goes through the engine of the batched front end (mut_pairs.cpp) as a list of one: every .mut file parsed in
    // parallel, the .colate.in files mapped, the SNP walk on one thread and the age sampling of the genome blocks on all the
    // others (or on the GPU), exact table-driven age bins -- the same tables bit for bit (22 x 1M rows: 3.3 -> 0.x s of table
    // fill, profiles/r04/bench/e2e_large.txt).  COLATE_THREADS=1: the sequential feeder, which is also what the engine falls
    // back to.
    const char* thr_env = std::getenv("COLATE_THREADS");
    if (thr_env && std::atoi(thr_env) <= 1) {
      fill_tables_from_tmp(names, mut_files, pair.target, pair.reference, pair.target_masks, pair.ref_masks, C, rng,
                           num_bases_per_block, A, tab);
    } else {
      for (size_t chr = 0; chr < mut_files.size(); chr++) std::cerr << "parsing CHR: " << chr + 1 << " / " << mut_files.size() << std::endl;
      std::vector<PairTables> tabs;
      fill_pairs(opt, names, mut_files, one, {0}, seed, A, tabs);
      tab = std::move(tabs[0]);
      rng = tab.rng;
    }
    const int nb = tab.nb;
    std::cerr << "Number of blocks: " << nb << std::endl;
    if (nb < 1) {
      std::cerr << "Error: no genome blocks were read." << std::endl;
      return 1;
    }
    num_blocks = nb;
    csh.assign((size_t)B * A, 0.0);
    cns.assign((size_t)B * A, 0.0);
    // the weights come from the run's mt19937 either way (coal.cpp:3350-3357); the weighted sums and
    // the F redistribution run on the GPU together with the EM unless only the counts are wanted
    // (--counts_only, no device needed) or the replicates are sharded over several GPUs
    gpu_bootstrap = !opt.has("counts_only") && !opt.has("devices") && !(g_rank.ranked && opt.has("counts_out")) &&
                    !opt.has("write_colate_mat");
    if (gpu_bootstrap) {
      weights.resize((size_t)B * nb);
      if (int rc = colate_bootstrap_weights(&rng, B, nb, weights.data())) return api_error(rc);
    } else if (int rc = colate_bootstrap_counts(&rng, B, nb, A, age_grid.data(), age, tab.sh.data(), tab.ns.data(),
                                                tab.she.data(), tab.nse.data(), csh.data(), cns.data())) {
      return api_error(rc);
    }
  } else {
    std::cerr << "Error: colate_amd reads --target_tmp/--reference_tmp (.colate.in) inputs or an "
                 "existing <output>.colate_mat; BCF/BAM inputs go through `Colate --mode make_tmp` first."
              << std::endl;
    return 1;
  }

  auto write_counts = [&]() {  // same layout as the reference's .colate_mat (coal.cpp:3336-3343, 3453-3469)
    write_counts_file(opt.get("counts_out"), B, A, age_grid, csh.data(), cns.data());
  };
  if (opt.has("write_colate_mat") && num_blocks > 0) {
    // coal.cpp:3336-3343, 3453-3470 (what the reference does when its inputs are BCF/BAM files): the counts are divided
    // by 1e3 IN PLACE -- the EM then runs on the scaled tables -- and written with the stream's default 6 significant
    // digits: grid line, then per replicate a line of shared and a line of not-shared counts.  The file is what a later
    // run (ours or the reference's) picks up as "precomputed file" (coal.cpp:3471-3499).
    const double norm = 1e3;
    for (double& v : csh) v /= norm;
    for (double& v : cns) v /= norm;
    if (g_rank.rank == 0) {
      std::ofstream os_mat(mat);
      for (int b = 0; b < A; b++) os_mat << age_grid[b] << " ";
      os_mat << "\n";
      for (int i = 0; i < B; i++) {
        for (int b = 0; b < A; b++) os_mat << csh[(size_t)i * A + b] << " ";
        os_mat << "\n";
        for (int b = 0; b < A; b++) os_mat << cns[(size_t)i * A + b] << " ";
        os_mat << "\n";
      }
    }
  }
  if (opt.has("counts_out") && !gpu_bootstrap) {
    if (g_rank.rank == 0) write_counts();
  }
  auto report_times = [&]() {
    if (g_times.on)
      std::cerr << "Timing: parse_mut " << g_times.parse_mut << " s, table_fill " << g_times.table_fill << " s, bootstrap_em "
                << g_times.bootstrap_em << " s" << std::endl;
  };
  if (opt.has("counts_only")) {
    report_times();
    return 0;
  }

  // ---- epochs (coal.cpp:3501-3646)
  if (!opt.has("coal") && !opt.has("bins")) {
    std::cerr << "Error: need --bins or --coal." << std::endl;
    return 1;
  }
  std::vector<double> epochs, init_rates;
  int ep_null = 0;
  const int E = pair_epochs(opt, opt.has("coal") ? &opt.get("coal") : nullptr, age, run.years_per_gen, epochs, init_rates, ep_null);
  if (E <= 0) {
    std::cerr << colate_last_error() << std::endl;
    return 1;
  }
  if (opt.has("coal")) {
    for (double r : init_rates) std::cerr << r << " ";
    std::cerr << std::endl;
  }

  std::cerr << "Maximising likelihood using EM.. " << std::endl;
  std::vector<int> devs;
  if (!bind_devices(opt, devs)) return 1;
  std::vector<double> rates((size_t)B * E), ll(B);
  std::vector<int> iters(B), flags(B);
  int rc;
  const double t_em0 = StageTimes::now();
  if (g_rank.ranked) {
    // one process per GPU: this rank's contiguous replicate range on its own device, then ONE RCCL all-gather
    RankComm comm;
    if (!comm.open(opt)) return 1;
    if (gpu_bootstrap)
      rc = colate_bootstrap_em_batch_allgather(comm.comm, B, num_blocks, E, A, age_grid.data(), age, weights.data(), tab.sh.data(),
                                               tab.ns.data(), tab.she.data(), tab.nse.data(), epochs.data(), init_rates.data(),
                                               COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL,
                                               COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(), ll.data(), flags.data());
    else
      rc = colate_em_batch_allgather(comm.comm, B, E, A, age_grid.data(), csh.data(), cns.data(), epochs.data(),
                                     init_rates.data(), COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER,
                                     COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(),
                                     ll.data(), flags.data());
    if (rc) return api_error(rc);
    if (g_rank.rank != 0) return 0;  // every rank holds all results; rank 0 reports and writes them
  } else if (!devs.empty()) {
    rc = colate_em_batch_sharded((int)devs.size(), devs.data(), B, E, A, age_grid.data(), csh.data(), cns.data(),
                                 epochs.data(), init_rates.data(), COLATE_DEFAULT_MAX_ITER,
                                 COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR,
                                 rates.data(), iters.data(), ll.data(), flags.data());
  } else if (gpu_bootstrap) {
    rc = colate_bootstrap_em_batch(B, num_blocks, E, A, age_grid.data(), age, weights.data(), tab.sh.data(), tab.ns.data(),
                                   tab.she.data(), tab.nse.data(), epochs.data(), init_rates.data(), COLATE_DEFAULT_MAX_ITER,
                                   COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR,
                                   rates.data(), iters.data(), ll.data(), flags.data(), csh.data(), cns.data());
    if (rc == 0 && opt.has("counts_out")) write_counts();
  } else {
    rc = colate_em_batch(B, E, A, age_grid.data(), csh.data(), cns.data(), epochs.data(),
                         init_rates.data(), COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER,
                         COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(),
                         iters.data(), ll.data(), flags.data());
  }
  g_times.bootstrap_em = StageTimes::now() - t_em0;
  report_times();
  if (rc) return api_error(rc);
  report_replicates(0, B, E, iters.data(), flags.data());
  if (colate_write_coal((out + ".coal").c_str(), B, E, epochs.data(), rates.data(), is_ancient ? 1 : 0, ep_null)) {
    std::cerr << "Error: " << colate_last_error() << std::endl;
    return 1;
  }

  print_usage_footer();
  return 0;
}

// Everything of a run over a list of pairs but the list and the table fill: epochs per pair, classes by number of epochs,
// bootstrap weights from each pair's generator, counts, the EM launches and the writers.  fill(todo, seed, A, tabs): the tables
// of the pairs listed in `todo` and each one's generator after its fill, as fill_pairs leaves them.
using PairListFill = std::function<bool(const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& tabs)>;
int run_pair_list(const Options& opt, const std::vector<PairSpec>& pairs, const PairListFill& fill);

int run_mut_pairs(const Options& opt) {
  if (!opt.has("mut")) {
    std::cerr << "Error: --pairs needs --mut (and optionally --chr, --bins, --num_bootstraps, --seed)." << std::endl;
    return 1;
  }
  for (const char* o : {"target_mask", "reference_mask", "coal"})
    if (opt.has(o)) {  // one mask / one warm start cannot mean the same for a whole list of pairs: refuse, do not ignore
      std::cerr << "Error: --" << o << " cannot be combined with --pairs (give it per line: " << o << "=...)." << std::endl;
      return 1;
    }
  std::vector<std::string> chr_names, mut_files;
  chromosome_files(opt, chr_names, mut_files);  // (once: the list's mask prefixes expand with these names, and the fill reads these files)
  std::vector<PairSpec> pairs;
  if (!read_pair_list(opt.get("pairs"), opt, chr_names, pairs)) return 1;
  if (!opt.has("bins"))
    for (size_t p = 0; p < pairs.size(); p++)
      if (pairs[p].coal.empty()) {  // (a line with coal= takes its epochs from that file)
        std::cerr << "Error: --pairs needs --bins for pair " << p + 1 << " (it names no coal= file)." << std::endl;
        return 1;
      }
  return run_pair_list(opt, pairs, [&](const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& tabs) {
    return fill_pairs(opt, chr_names, mut_files, pairs, todo, seed, A, tabs);
  });
}

int run_pair_list(const Options& opt, const std::vector<PairSpec>& pairs, const PairListFill& fill) {
  const bool talk = g_rank.rank == 0;
  if (talk) {
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Calculating coalescence rates for " << pairs.size() << " pairs of (ancient) samples.." << std::endl;
  }
  RunSetup run(opt);
  if (!run.read_replicates(opt)) return 1;
  const int A = run.A, B = run.B;
  const std::vector<double>& age_grid = run.age_grid;
  const size_t P = pairs.size();
  const bool counts_only = opt.has("counts_only");
  const bool want_counts = counts_only || opt.has("counts_out");
  const DeviceWarmUp warm(opt);

  // ---- epochs per pair (coal.cpp:3501-3632): from the ages and --bins, or from the pair's coal= file (which also gives its
  // starting rates, coal.cpp:3638-3646): the launches are known before any file is read
  std::vector<std::vector<double>> epochs(P), init(P);
  std::vector<int> ep_null(P, 0);
  std::vector<double> age(P);
  for (size_t p = 0; p < P; p++) {
    age[p] = std::max(pairs[p].target_age, pairs[p].ref_age) / run.years_per_gen;
    const std::string* coal = pairs[p].coal.empty() ? nullptr : &pairs[p].coal;
    if (pair_epochs(opt, coal, age[p], run.years_per_gen, epochs[p], init[p], ep_null[p]) <= 0) {
      std::cerr << "Error: pair " << p + 1 << ": " << colate_last_error() << std::endl;
      return 1;
    }
    if (coal && talk) {  // (as the single-pair CLI prints them, after the pair's number)
      std::cerr << "Pair " << p + 1 << ": ";
      for (double r : init[p]) std::cerr << r << " ";
      std::cerr << std::endl;
    }
  }
  // classes of pairs with the same number of epochs, in order of first appearance: one launch each
  std::vector<std::vector<size_t>> classes;
  for (size_t p = 0; p < P; p++) {
    size_t c = 0;
    while (c < classes.size() && epochs[classes[c][0]].size() != epochs[p].size()) c++;
    if (c == classes.size()) classes.emplace_back();
    classes[c].push_back(p);
  }
  // --ranks N: this rank's rows [lo, hi) of every class (row = position in the class * B + replicate) and the pairs they belong to
  std::vector<size_t> todo;
  std::vector<int> first_group(classes.size(), 0), group_count(classes.size(), 0);
  for (size_t c = 0; c < classes.size(); c++) {
    const int R = (int)(classes[c].size() * (size_t)B);
    int lo = 0, hi = R;
    if (g_rank.ranked) colate_shard_bounds(R, g_rank.nranks, g_rank.rank, &lo, &hi);
    if (counts_only && g_rank.ranked && g_rank.rank != 0) lo = hi = 0;
    if (hi > lo) {
      first_group[c] = lo / B;
      group_count[c] = (hi - 1) / B - lo / B + 1;
      for (int g = 0; g < group_count[c]; g++) todo.push_back(classes[c][(size_t)(first_group[c] + g)]);
    }
  }
  std::sort(todo.begin(), todo.end());

  std::vector<PairTables> tabs;
  if (!fill(todo, run.seed, A, tabs)) return 1;
  for (size_t p : todo) {
    if (talk) std::cerr << "Pair " << p + 1 << " / " << P << ": " << pairs[p].target << " x " << pairs[p].reference << ": Number of blocks: " << tabs[p].nb << std::endl;
    if (tabs[p].nb < 1) {
      std::cerr << "Error: no genome blocks were read for pair " << p + 1 << "." << std::endl;
      return 1;
    }
  }
  // ---- bootstrap weights from each pair's own generator (coal.cpp:3350-3357)
  std::vector<std::vector<double>> weights(P);
  for (size_t p : todo) {
    weights[p].resize((size_t)B * tabs[p].nb);
    if (int rc = colate_bootstrap_weights(&tabs[p].rng, B, tabs[p].nb, weights[p].data())) return api_error(rc);
  }
  if (counts_only) {  // no device: the weighted sums and the F redistribution on the host (coal.cpp:3358-3451)
    for (size_t p : todo) {
      std::vector<double> csh((size_t)B * A), cns((size_t)B * A);
      PairTables& pt = tabs[p];
      if (int rc = colate_bootstrap_counts_from_weights(B, pt.nb, A, age_grid.data(), age[p], weights[p].data(), pt.sh.data(),
                                                        pt.ns.data(), pt.she.data(), pt.nse.data(), csh.data(), cns.data()))
        return api_error(rc);
      write_counts_file(pairs[p].output + ".counts", B, A, age_grid, csh.data(), cns.data());
    }
    return 0;
  }

  if (talk) std::cerr << "Maximising likelihood using EM.. " << std::endl;
  std::vector<int> dev_list;
  if (!bind_devices(opt, dev_list)) return 1;
  RankComm comm;
  if (g_rank.ranked && !comm.open(opt)) return 1;
  const double t_em0 = StageTimes::now();
  int status = 0;
  for (size_t c = 0; c < classes.size() && status == 0; c++) {
    const std::vector<size_t>& cls = classes[c];
    const int G = (int)cls.size(), E = (int)epochs[cls[0]].size();
    const size_t R = (size_t)G * B;
    const int g0 = first_group[c], gn = group_count[c];
    // this process's groups of the class, concatenated
    std::vector<int> nb(gn);
    std::vector<double> g_age(gn), g_w, g_sh, g_ns, g_she, g_nse, g_ep((size_t)gn * E), g_init((size_t)gn * E);
    for (int g = 0; g < gn; g++) {
      const size_t p = cls[(size_t)(g0 + g)];
      const PairTables& pt = tabs[p];
      nb[g] = pt.nb, g_age[g] = age[p];
      g_w.insert(g_w.end(), weights[p].begin(), weights[p].end());
      g_sh.insert(g_sh.end(), pt.sh.begin(), pt.sh.end());
      g_ns.insert(g_ns.end(), pt.ns.begin(), pt.ns.end());
      g_she.insert(g_she.end(), pt.she.begin(), pt.she.end());
      g_nse.insert(g_nse.end(), pt.nse.begin(), pt.nse.end());
      std::copy(epochs[p].begin(), epochs[p].end(), g_ep.begin() + (size_t)g * E);
      std::copy(init[p].begin(), init[p].end(), g_init.begin() + (size_t)g * E);
    }
    std::vector<double> rates(R * E), ll(R), csh, cns;
    std::vector<int> iters(R), flags(R);
    if (want_counts) csh.resize(R * A), cns.resize(R * A);
    int rc;
    if (g_rank.ranked) {
      rc = colate_bootstrap_em_batch_groups_allgather(comm.comm, G, B, g0, gn, E, A, age_grid.data(), nb.data(), g_age.data(), g_w.data(),
                                                      g_sh.data(), g_ns.data(), g_she.data(), g_nse.data(), g_ep.data(), g_init.data(),
                                                      COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL,
                                                      COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(), ll.data(), flags.data());
    } else if (!dev_list.empty()) {
      // --devices N (one process, several GPUs): counts on the host, the rows sharded over GPUs 0..N-1
      csh.resize(R * A), cns.resize(R * A);
      rc = 0;
      for (int g = 0, wo = 0, bo = 0; g < G && !rc; wo += B * nb[g], bo += nb[g], g++)
        rc = colate_bootstrap_counts_from_weights(B, nb[g], A, age_grid.data(), g_age[g], g_w.data() + wo, g_sh.data() + (size_t)bo * A,
                                                  g_ns.data() + (size_t)bo * A, g_she.data() + (size_t)bo * A, g_nse.data() + (size_t)bo * A,
                                                  csh.data() + (size_t)g * B * A, cns.data() + (size_t)g * B * A);
      std::vector<double> r_ep(R * E), r_init(R * E);
      colate::expand_group_rows(g_ep.data(), (int)B, 0, 0, (long)R, E, r_ep.data());
      colate::expand_group_rows(g_init.data(), (int)B, 0, 0, (long)R, E, r_init.data());
      if (!rc)
        rc = colate_em_batch_rows_sharded((int)dev_list.size(), dev_list.data(), (int)R, E, A, age_grid.data(), csh.data(), cns.data(),
                                          r_ep.data(), r_init.data(), COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER,
                                          COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(), ll.data(),
                                          flags.data());
    } else {
      rc = colate_bootstrap_em_batch_groups(G, B, E, A, age_grid.data(), nb.data(), g_age.data(), g_w.data(), g_sh.data(), g_ns.data(),
                                            g_she.data(), g_nse.data(), g_ep.data(), g_init.data(), COLATE_DEFAULT_MAX_ITER,
                                            COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(),
                                            iters.data(), ll.data(), flags.data(), want_counts ? csh.data() : nullptr,
                                            want_counts ? cns.data() : nullptr);
    }
    if (rc) {
      status = api_error(rc);
      break;
    }
    if (!talk) continue;
    for (int g = 0; g < G; g++) {
      const size_t p = cls[(size_t)g];
      report_replicates((int)p + 1, B, E, iters.data() + (size_t)g * B, flags.data() + (size_t)g * B);
      if (want_counts && !csh.empty())
        write_counts_file(pairs[p].output + ".counts", B, A, age_grid, csh.data() + (size_t)g * B * A, cns.data() + (size_t)g * B * A);
      if (colate_write_coal((pairs[p].output + ".coal").c_str(), B, E, epochs[p].data(), rates.data() + (size_t)g * B * E,
                            age[p] > 0.0 ? 1 : 0, ep_null[p])) {
        std::cerr << "Error: " << colate_last_error() << std::endl;
        status = 1;
        break;
      }
    }
  }
  g_times.bootstrap_em = StageTimes::now() - t_em0;
  if (g_times.on)
    std::cerr << "Timing: inputs " << g_times.parse_mut << " s, pairs' table fill " << g_times.table_fill << " s, bootstrap_em "
              << g_times.bootstrap_em << " s" << std::endl;
  if (status || !talk) return status;
  print_usage_footer();
  return 0;
}

// `Colate --mode mut --samples LIST`: every (target line, reference line) of the list, each pair's files byte for byte what
// `--pairs` writes for the expanded list.  The tables come from fill_sample_pairs (fill_samples.cpp): walked and filled on the
// device where there is one, else through fill_pairs.
int run_mut_samples(const Options& opt) {
  for (const char* o : {"pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "ranks"})
    if (opt.has(o)) {
      std::cerr << "Error: --" << o << " cannot be combined with --mode mut --samples." << std::endl;
      return 1;
    }
  if (!opt.has("mut") || !opt.has("output") || (!opt.has("bins") && !opt.has("coal"))) {
    std::cerr << "Error: --samples needs --mut, -o PREFIX and --bins x,y,stepsize or --coal FILE (optional: --chr, --num_bootstraps, --seed, "
                 "--years_per_gen, --counts_out, --counts_only, --device, --devices)."
              << std::endl;
    return 1;
  }
  std::vector<std::string> chr_names, mut_files;
  chromosome_files(opt, chr_names, mut_files);
  std::vector<SampleLine> samples;
  if (!read_sample_list(opt.get("samples"), opt, chr_names, true, samples)) return 1;
  std::vector<PairSpec> pairs;
  for (const SampleLine& t : samples)
    for (const SampleLine& r : samples) {
      if (!t.target || !r.reference || &t == &r) continue;
      PairSpec ps;
      ps.target = t.file, ps.reference = r.file, ps.output = opt.get("output") + "_" + t.name + "_" + r.name;
      ps.target_age = t.age, ps.ref_age = r.age, ps.target_masks = t.masks, ps.ref_masks = r.masks, ps.line = t.line;
      if (!opt.has("bins")) ps.coal = opt.get("coal");
      pairs.push_back(ps);
    }
  if (pairs.empty()) {
    std::cerr << "Error: " << opt.get("samples") << ": no pair of a target and a reference on different lines." << std::endl;
    return 1;
  }
  return run_pair_list(opt, pairs, [&](const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& tabs) {
    return fill_sample_pairs(opt, chr_names, mut_files, pairs, todo, seed, A, tabs);
  });
}

void write_counts_file(const std::string& path, int B, int A, const std::vector<double>& grid,
                       const double* csh, const double* cns) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) {
    std::cerr << "Error: cannot write " << path << std::endl;
    std::exit(1);
  }
  for (int b = 0; b < A; b++) std::fprintf(f, "%.17g ", grid[b]);
  std::fprintf(f, "\n");
  for (int i = 0; i < B; i++) {
    for (int b = 0; b < A; b++) std::fprintf(f, "%.17g ", csh[(size_t)i * A + b]);
    std::fprintf(f, "\n");
    for (int b = 0; b < A; b++) std::fprintf(f, "%.17g ", cns[(size_t)i * A + b]);
    std::fprintf(f, "\n");
  }
  std::fclose(f);
}

// ------------------------------------------------------------------ --mode make_tmp --target_table
// The htslib-free input of the reference's make_tmp (coal.cpp:2923-3069 -> maketmp_table, coal.cpp:2682-2808): a text
// table `chr bp allele` of the target's haploid calls becomes the binary .colate.in stream `--mode mut` reads
// (record layout coal.cpp:2505-2514).  BCF and BAM inputs (maketmp_vcf / maketmp_bam) need htslib and stay with the
// reference build.  The table is walked with formatted extraction exactly like the reference's igzstream (a failed
// read at the end of the file leaves the last record in place).
int run_make_tmp(const Options& opt) {
  if (!opt.has("mut") || !opt.has("output")) {  // coal.cpp:2929-2939
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: mut, ref_genome, output, either of target_bcf or target_bam. Optional: filters, target_mask, "
                 "strandfilter, anc_genome."
              << std::endl;
    print_help();
    std::cout << "Calculate coalescence rates for sample." << std::endl;
    return 0;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating Colate tmp input file for ";
  if (opt.has("target_bcf") || opt.has("target_bam")) {
    std::cerr << std::endl
              << "Error: colate_amd's make_tmp reads --target_table only; BCF/BAM inputs need htslib (reference build)."
              << std::endl;
    return 1;
  }
  if (!opt.has("target_table")) {  // (the reference falls through and writes nothing)
    std::cerr << std::endl << "Error: --mode make_tmp needs --target_table." << std::endl;
    return 1;
  }
  if (!opt.has("ref_genome")) {  // cxxopts throws on options["ref_genome"].as<std::string>() (coal.cpp:3027, 3037)
    std::cerr << std::endl << "Error: --mode make_tmp --target_table needs --ref_genome." << std::endl;
    return 1;
  }
  std::cerr << opt.get("target_table") << ".." << std::endl;
  std::vector<std::string> names, mut_files, ref_genomes, tmasks;
  if (opt.has("chr")) {  // coal.cpp:3018-3032
    GzText is_chr;
    if (!is_chr.open(opt.get("chr"))) std::cerr << "Error while opening file " << opt.get("chr") << std::endl;
    std::string line;
    while (is_chr.getline(line)) {
      names.push_back(line);
      mut_files.push_back(opt.get("mut") + "_chr" + line + ".mut");
      ref_genomes.push_back(opt.get("ref_genome") + "_chr" + line + ".fa");
      if (opt.has("target_mask")) tmasks.push_back(opt.get("target_mask") + "_chr" + line + ".fa");
    }
  } else {
    names.push_back("");
    mut_files.push_back(opt.get("mut"));
    ref_genomes.push_back(opt.get("ref_genome"));
    if (opt.has("target_mask")) tmasks.push_back(opt.get("target_mask"));
  }
  const std::string out_name = opt.get("output") + ".colate.in";
  FILE* fp = std::fopen(out_name.c_str(), "wb");
  if (!fp) {
    std::cerr << "Error: cannot write " << out_name << std::endl;
    return 1;
  }
  std::istringstream is;
  {
    GzText table;
    if (!table.open(opt.get("target_table"))) {  // coal.cpp:2699-2702
      std::cerr << "Error while opening file " << opt.get("target_table") << std::endl;
      return 1;
    }
    std::string all, line;
    while (table.getline(line)) {
      all += line;
      all += '\n';
    }
    is.str(all);
  }
  const bool has_tar_mask = !tmasks.empty();
  std::string chr_table, allele, ancestral, derived;
  int bp_target = -1;
  const int N_target = 1;
  for (size_t chr = 0; chr < mut_files.size(); chr++) {
    std::cerr << "parsing CHR: " << chr + 1 << " / " << mut_files.size() << std::endl;
    std::string tar_mask, ref_genome;
    if (has_tar_mask) read_fasta_mask(tmasks[chr], tar_mask);
    std::vector<MutRow> rows;
    read_mut_file(mut_files[chr], rows);
    read_fasta_mask(ref_genomes[chr], ref_genome);  // read (and required to exist) as in the reference; only its presence matters
    if (bp_target == -1) is >> chr_table >> bp_target >> allele;
    while (chr_table != names[chr]) {
      if (!(is >> chr_table >> bp_target >> allele)) break;
    }
    for (const MutRow& m : rows) {
      if (m.flipped != 0 || m.num_branches != 1) continue;
      size_t i = 0;
      ancestral.clear();
      derived.clear();
      while (i < m.mutation_type.size() && m.mutation_type[i] != '/') ancestral.push_back(m.mutation_type[i++]);
      i++;
      while (i < m.mutation_type.size()) derived.push_back(m.mutation_type[i++]);
      const int bp_mut = m.pos;
      if (ancestral.empty() || derived.empty()) continue;
      bool use = true;
      if (ancestral != "A" && ancestral != "C" && ancestral != "G" && ancestral != "T" && ancestral != "0") use = false;
      if (derived != "A" && derived != "C" && derived != "G" && derived != "T" && derived != "1") use = false;
      if (has_tar_mask) {  // coal.cpp:2749-2755: sites beyond the mask are dropped here (unlike in parse_tmptmp)
        if (bp_mut >= (int)tar_mask.size())
          use = false;
        else if (bp_mut < 1 || tar_mask[bp_mut - 1] != 'P')
          use = false;
      }
      if (!use) continue;
      if (chr_table == names[chr] && bp_target < bp_mut) {
        while (!is.eof() && chr_table == names[chr] && bp_target < bp_mut) is >> chr_table >> bp_target >> allele;
      }
      int DAF_target = 0;
      if (chr_table == names[chr] && bp_target == bp_mut) {  // the target has a call here (coal.cpp:2768-2782)
        if (allele == derived || allele == ancestral) {
          if (allele == derived) DAF_target = 1;
        } else {
          use = false;
        }
      } else {
        use = false;
      }
      if (!use) continue;
      const int lchrom = (int)names[chr].size();
      const int AAF_target = N_target - DAF_target;
      std::fwrite(&lchrom, sizeof(int), 1, fp);
      std::fwrite(names[chr].c_str(), sizeof(char), (size_t)lchrom, fp);
      std::fwrite(&bp_mut, sizeof(int), 1, fp);
      std::fwrite(&ancestral[0], sizeof(char), 1, fp);
      std::fwrite(&derived[0], sizeof(char), 1, fp);
      std::fwrite(&AAF_target, sizeof(int), 1, fp);
      std::fwrite(&DAF_target, sizeof(int), 1, fp);
    }
  }
  std::fclose(fp);
  print_usage_footer();  // coal.cpp:3055-3067
  return 0;
}

// `--ranks N`: fork N processes BEFORE anything touches the GPU (this process never does), one per GPU; each runs the
// whole `--mode mut` pipeline (same inputs, same --seed, hence the same tables and bootstrap weights), computes its
// contiguous range of replicates and takes part in one RCCL all-gather (colate_comm.cpp); rank 0 writes the outputs.
// The launcher only relays rank 0's 128-byte communicator id to the other ranks and collects the exit codes.
int run_ranked(const Options& opt, int nranks) {
  if (colate_device_touched()) {
    // fork() after the HIP runtime is up gives children with a half-copied runtime (its threads and device queues are
    // not duplicated): they hang or fault.  The command-line `Colate` never gets here; a host process that has already
    // computed through this library (or that shares it with torch) must start the ranks as fresh processes instead.
    std::cerr << "Error: --ranks forks one process per GPU and must run before this process first uses a GPU through "
                 "libcolate_amd; start `Colate --ranks N` as its own process (never re-exec from here)." << std::endl;
    return 1;
  }
  if (!opt.has("seed")) {
    std::cerr << "Error: --ranks needs --seed (every rank must draw the same bootstrap weights)." << std::endl;
    return 1;
  }
  if (opt.has("devices")) {
    std::cerr << "Error: --ranks cannot be combined with --devices." << std::endl;
    return 1;
  }
  if (opt.has("pairs") && opt.has("counts_out") && !opt.has("counts_only")) {
    // (the ranks all-gather the rates, not the counts; --counts_only computes every pair's counts on rank 0)
    std::cerr << "Error: --ranks cannot write the .counts files of a --pairs list (--counts_out) unless --counts_only is given."
              << std::endl;
    return 1;
  }
  // where the ranks other than 0 keep their progress lines: next to the output (with --pairs: next to the list of pairs)
  const std::string log_prefix = opt.has("pairs") ? opt.get("pairs") : opt.get("output");
  int up[2];
  if (::pipe(up) != 0) {
    std::perror("pipe");
    return 1;
  }
  std::vector<int> down_r(nranks, -1), down_w(nranks, -1);
  for (int r = 1; r < nranks; r++) {
    int fd[2];
    if (::pipe(fd) != 0) {
      std::perror("pipe");
      return 1;
    }
    down_r[r] = fd[0], down_w[r] = fd[1];
  }
  std::cerr.flush();
  std::cout.flush();
  std::vector<pid_t> pids(nranks, -1);
  for (int r = 0; r < nranks; r++) {
    pid_t pid = ::fork();
    if (pid < 0) {
      std::perror("fork");
      return 1;
    }
    if (pid == 0) {  // rank r
      g_rank.ranked = true, g_rank.rank = r, g_rank.nranks = nranks;
      ::close(up[0]);
      for (int q = 1; q < nranks; q++) {
        ::close(down_w[q]);
        if (q != r) ::close(down_r[q]);
      }
      if (r == 0) {
        g_rank.fd_id_out = up[1];
      } else {
        ::close(up[1]);
        g_rank.fd_id_in = down_r[r];
        // only rank 0 talks on the terminal; the others keep their progress lines in a file that a clean exit removes
        const std::string log = log_prefix + ".rank" + std::to_string(r) + ".stderr";
        if (!std::freopen(log.c_str(), "w", stderr)) std::perror("freopen");
      }
      int code = 1;
      try {
        code = opt.has("pairs") ? run_mut_pairs(opt) : run_mut(opt);
      } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << std::endl;
      }
      std::cerr.flush();
      if (r != 0 && code == 0) std::remove((log_prefix + ".rank" + std::to_string(r) + ".stderr").c_str());
      std::fflush(nullptr);
      ::_exit(code);
    }
    pids[r] = pid;
  }
  ::close(up[1]);
  for (int r = 1; r < nranks; r++) ::close(down_r[r]);
  // One loop relays rank 0's communicator id to the other ranks AND reaps the ranks as they end (our own pids only: this
  // function is also reachable through the library ABI, whose host may have children of its own).  Nothing here blocks:
  //  * a rank that fails before or outside the collective leaves the others waiting in ncclCommInitRank / ncclAllGather
  //    for ever, so the first failure -- or any exit while the id is still outstanding -- starts a grace period
  //    (COLATE_RANK_GRACE_SEC, default 15 s: ranks that are merely finishing get there) after which the rest are killed;
  //  * rank 0 ending without having published the id closes the other ranks' pipes (they report and exit);
  //  * a rank 0 that neither publishes the id nor ends (stuck in HIP initialisation, ncclGetUniqueId or its table fill)
  //    is given COLATE_RANK_ID_TIMEOUT_SEC (default 3600 s: the id follows the table fill, which may be long), then
  //    every rank is killed and the launcher returns non-zero.
  double grace_s = 15.0, id_timeout_s = 3600.0;
  if (const char* g = std::getenv("COLATE_RANK_GRACE_SEC")) grace_s = std::atof(g);
  if (const char* g = std::getenv("COLATE_RANK_ID_TIMEOUT_SEC")) id_timeout_s = std::atof(g);
  unsigned char id[COLATE_COMM_ID_BYTES];
  size_t id_have = 0;
  bool id_open = true;
  auto close_id_pipes = [&]() {
    if (!id_open) return;
    ::close(up[0]);
    for (int r = 1; r < nranks; r++) ::close(down_w[r]);
    id_open = false;
  };
  ::fcntl(up[0], F_SETFL, ::fcntl(up[0], F_GETFL, 0) | O_NONBLOCK);
  const auto t_start = std::chrono::steady_clock::now();
  auto seconds_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
  };
  int worst = 0, remaining = nranks;
  std::vector<char> done(nranks, 0);
  bool failing = false, killed = false;
  auto t_fail = std::chrono::steady_clock::now();
  auto kill_rest = [&]() {
    for (int r = 0; r < nranks; r++)
      if (!done[r]) ::kill(pids[r], SIGKILL);
    killed = true;
  };
  while (remaining > 0) {
    bool progressed = false;
    if (id_open) {  // (waits up to 20 ms for bytes of the id: this is also the loop's pause)
      pollfd pfd{up[0], POLLIN, 0};
      if (::poll(&pfd, 1, 20) > 0) {
        const ssize_t k = ::read(up[0], id + id_have, sizeof(id) - id_have);
        if (k > 0) {
          id_have += (size_t)k;
          if (id_have == sizeof(id)) {
            for (int r = 1; r < nranks; r++) write_all(down_w[r], id, sizeof(id));
            close_id_pipes();
          }
          progressed = true;
        } else if (k == 0) {  // rank 0 ended (or closed its end) without an id: end-of-file for the others, too
          close_id_pipes();
        }
      }
      if (id_open && !killed && seconds_since(t_start) > id_timeout_s) {
        std::cerr << "Error: rank 0 has not published the communicator id after " << id_timeout_s
                  << " s (COLATE_RANK_ID_TIMEOUT_SEC); ending all ranks." << std::endl;
        close_id_pipes();
        kill_rest();
        worst = 1;
      }
    }
    for (int r = 0; r < nranks; r++) {
      if (done[r]) continue;
      int st = 0;
      const pid_t w = ::waitpid(pids[r], &st, WNOHANG);
      if (w == 0) continue;
      done[r] = 1, remaining--, progressed = true;
      const bool ok = (w == pids[r]) && WIFEXITED(st) && WEXITSTATUS(st) == 0;
      if (!ok) {
        std::cerr << "Error: rank " << r << (killed ? " was ended by the launcher" : " failed");
        if (r > 0) std::cerr << " (see " << log_prefix << ".rank" << r << ".stderr)";
        std::cerr << std::endl;
        worst = 1;
      }
      // a failure -- or any exit while the id is outstanding (nobody can finish properly without it) -- starts the clock
      if ((!ok || (id_open && nranks > 1)) && !failing) failing = true, t_fail = std::chrono::steady_clock::now();
    }
    if (remaining == 0) break;
    if (failing && !killed && seconds_since(t_fail) > grace_s) {
      std::cerr << "Error: a rank failed; ending the " << remaining << " rank(s) still waiting after " << grace_s << " s."
                << std::endl;
      close_id_pipes();
      kill_rest();
      worst = 1;
    }
    if (!progressed && !id_open) ::usleep(20000);
  }
  close_id_pipes();
  return worst;
}

}  // namespace colate_drv

using namespace colate_drv;

extern "C" int colate_mut_main(int argc, char** argv) {
  Options opt;
  std::string err;
  if (!parse_options(argc, argv, opt, err)) {
    std::cerr << err << std::endl;
    return 1;
  }
  if (!opt.has("mode")) {  // Colate.cpp:104-112
    std::cout << "Not enough arguments supplied." << std::endl;
    print_help();
    return 0;
  }
  const std::string& mode = opt.get("mode");
  for (const char* o : {"age_profile", "profile_only"})
    if (opt.has(o) && mode != "count_topo") {
      std::cerr << "Error: --" << o << " is an option of --mode count_topo --samples." << std::endl;
      return 1;
    }
  if (mode == "mut") {
    if (opt.has("help")) {
      print_help();
      std::cout << "Calculate coalescence rates for sample." << std::endl;
      return 0;
    }
    try {
      if (opt.has("samples")) return run_mut_samples(opt);  // (refuses --ranks by name)
      if (opt.has("ranks")) {
        const int nranks = std::stoi(opt.get("ranks"));
        if (nranks < 1 || nranks > 64) {
          std::cerr << "Error: --ranks must be between 1 and 64." << std::endl;
          return 1;
        }
        if (opt.has("mut") && (opt.has("output") || opt.has("pairs"))) return run_ranked(opt, nranks);  // (also for N = 1: same code path)
      }
      if (opt.has("pairs")) return run_mut_pairs(opt);
      return run_mut(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  if (mode == "mut_interval") {
    try {
      return run_mut_interval(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  if (mode == "compare_tmp") {
    try {
      return run_compare_tmp(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  if (mode == "count_topo") {
    try {
      return run_count_topo(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  if (mode == "make_tmp") {
    try {
      return run_make_tmp(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  if (mode == "CondCoalRates") {
    try {
      return run_condcoal(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  std::cout << "####### error #######" << std::endl;
  std::cout << "colate_amd implements --mode mut, --mode mut_interval, --mode compare_tmp, --mode count_topo, --mode make_tmp --target_table and --mode "
               "CondCoalRates (preprocess_mut, make_tmp from BCF/BAM, calc_depth, print_tmp stay with the reference build)."
            << std::endl;
  return 1;
}
