// driver.h -- polymutt-compatible command line and section/site loop (src/main.cpp:57-627),
// batching sites into dense blocks for a SiteEvaluator (the HIP engine in the product binary).
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/polymutt_engine.h"
#include "pedigree.h"

namespace pmhost {

struct Options {
  std::string pedFile, datFile, glfListFile, vcfOutFile, vcfInFile, positionFile, chrs2process;
  std::string chrX = "X", chrY = "Y", MT = "MT";
  double posterior = 0.5, theta = 0.001, theta_indel = 0.0001, tstv = 2.0, precision = 0.0001;
  int minTotalDepth = 0, maxTotalDepth = 0, minMapQuality = 0, nthreads = 1;
  double minPS = 0;
  bool denovo = false, gl_off = false, quick_call = false, all_sites = false, force_call = false, exact_log10 = false;
  std::string numerics = "poly";
  double denovo_rate = 1.5e-08, denovo_tstv = 2.0, denovo_llr = 0.01;
  int device = 0, batch = 4096;
  int engines = 2;      // --engines: engine instances (HIP streams) with a batch in flight each (pipelined CLI)
  int io_threads = 0;   // GLF decode threads (0: min(16, hardware threads))
  std::string blocksIn, blocksOut;   // --in_blocks FILE (.pmb input in place of -g), --glf2blocks FILE (convert)
  int blockSites = 4096;
  // --denovo_families K: de novo records name the K families (1..8) with the largest share of DQ (INFO tags DNF / DNFLR)
  int denovo_families = 0;
  bool denovo_families_given = false;
  // --denovo_carriers K: de novo records name the K non-founders (1..8) most likely to carry a de novo mutation, with
  // their posterior and most likely event (INFO tags DNC / DNCP / DNCE)
  int denovo_carriers = 0;
  bool denovo_carriers_given = false;
  // --vcf_denovo (with --in_vcf): biallelic autosomal SNV records whose three-genotype de novo model beats the standard
  // one by DQ >= --minLLR_denovo get ;DQ= after DP= (pm_engine_set_vcf_denovo; --rate_denovo, --tstv_denovo apply)
  bool vcf_denovo = false;
  // --vcf_denovo_families K / --vcf_denovo_carriers K (each with --vcf_denovo, K in 1..8): a record that gets ;DQ= also names
  // the K families with the largest share of DQ (DNF / DNFLR) and the K non-founders most likely to carry a de novo
  // mutation (DNC / DNCP / DNCE), in the formats of --denovo_families / --denovo_carriers (pm_engine_set_vcf_denovo_detail)
  int vcf_denovo_families = 0, vcf_denovo_carriers = 0;
  bool vcf_denovo_families_given = false, vcf_denovo_carriers_given = false;
  // --vcf_denovo_chrX (with --vcf_denovo): biallelic SNV records of the --chrX chromosome get ;DQ= too, from the sex-aware
  // three-state chrX model (pm_engine_set_vcf_denovo_chrx); DQ alone: the DNF / DNC detail stays autosomal only ...
  bool vcf_denovo_chrX = false;
  // ... unless --vcf_denovo_chrX_detail (with --vcf_denovo_chrX and --vcf_denovo_families and / or --vcf_denovo_carriers):
  // chrX SNV records that get ;DQ= get those tags too, from the same model (pm_engine_set_vcf_denovo_chrx_detail); in DNCE
  // a male's genotype is printed as its single allele, as the GT column prints him
  bool vcf_denovo_chrX_detail = false;
  // --vcf_posteriors (with --in_vcf): every sample of every written record also gets DS and GP, the dosage and the three
  // genotype posteriors given the pedigree behind its GT and GQ (pm_engine_set_vcf_posteriors); combines freely with the
  // --vcf_denovo flags
  bool vcf_posteriors = false;
  // --vcf_phase (with --in_vcf): a heterozygous non-founder of an autosomal record whose transmission phase is known with
  // a quality PQ >= --vcf_phase_minPQ (0..99, default 10) prints its GT phased, paternal allele first (0|1 or 1|0), and
  // every sample gets a PQ sub-field before PL / GL (pm_engine_set_vcf_phase); combines freely with the other --vcf_ flags
  bool vcf_phase = false;
  int vcf_phase_minPQ = 10;
  bool vcf_phase_minPQ_given = false;
  // --vcf_joint (with --in_vcf): every sample of every written record also gets JG and JL before PL / GL, its genotype in
  // its family's most probable joint (Mendelian-consistent) assignment and the log10 posterior of that assignment
  // (pm_engine_set_vcf_joint); GT stays the marginal call; combines freely with the other --vcf_ flags
  bool vcf_joint = false;
  // --vcf_pedcheck FILE (with --in_vcf): at the end of the run FILE gets, for every non-founder, the log10 likelihood ratio of
  // each stated parent link against an unrelated one, summed over the run's autosomal records (pm_engine_set_vcf_pedcheck);
  // the VCF output and stdout do not change; combines freely with the other --vcf_ flags
  std::string vcf_pedcheck;
  std::string cmd;
  pm_params params() const;
};

// Parses argv the way ParameterList does for the flags polymutt declares (main.cpp:88-134).
// Throws FatalError on unknown options.
Options parse_command_line(int argc, char** argv);

// The compute backend behind the drop-in boundary.
class SiteEvaluator {
 public:
  virtual ~SiteEvaluator() {}
  virtual void begin_section(int chrom) = 0;
  virtual void run(int n, const uint8_t* pl, const uint32_t* dm, const uint8_t* ref, pm_site_result* res, pm_geno_call* calls,
                   int* n_rows) = 0;
  // vcf_mode: the genotype rows in their compact form (pm_engine_run_vcf); the default runs run() and narrows them
  virtual void run_vcf(int n, int n_person, const uint8_t* pl, const uint8_t* ref, pm_site_result* res, pm_vcf_call* calls,
                       int* n_rows);
  virtual void counters(pm_counters* out) = 0;
  // famlk[0]'s stale posterior state at a shard start (pm_engine_set_posterior_carry)
  virtual void set_posterior_carry(bool seen) = 0;
  // Batches in flight (the pipelined CLI): submit() starts a batch -- res / calls are filled by the matching
  // collect(), which returns its row count; batches are collected in submission order, and at most in_flight()
  // are outstanding.  The default runs the batch inside submit().
  virtual int in_flight() const { return 1; }
  // (a BrentError of the batch surfaces at its collect(), after the batches before it, as the engine's does)
  virtual void submit(int n, const uint8_t* pl, const uint32_t* dm, const uint8_t* ref, pm_site_result* res, pm_geno_call* calls) {
    int rows = 0, valid = -1;
    try {
      run(n, pl, dm, ref, res, calls, &rows);
    } catch (const BrentError& e) {
      valid = e.valid;
      rows = e.rows;
    }
    done_.push_back({rows, valid});
  }
  virtual int collect() {
    const std::pair<int, int> d = done_.front();
    done_.erase(done_.begin());
    if (d.second >= 0) throw BrentError(d.second, d.first);
    return d.first;
  }
  // --denovo_families: set_denovo_families(K) once, before the first batch; then denovo_families(top) hands out the
  // rows [rows][K] (indexed by call_row) of the batch the last run() or collect() returned -- also after that call
  // threw a BrentError (the rows before the stuck site) -- and must be called before that batch's engine is given
  // another one.  Only the GPU engine computes them.
  virtual void set_denovo_families(int top_k) { (void)top_k; throw FatalError("--denovo_families needs the GPU engine\n"); }
  virtual void denovo_families(pm_fam_lr* top) { (void)top; throw FatalError("--denovo_families needs the GPU engine\n"); }
  // --denovo_carriers: the same protocol with the rows [rows][K] of ranked non-founders
  virtual void set_denovo_carriers(int top_k) { (void)top_k; throw FatalError("--denovo_carriers needs the GPU engine\n"); }
  virtual void denovo_carriers(pm_person_dn* top) { (void)top; throw FatalError("--denovo_carriers needs the GPU engine\n"); }
  // --vcf_denovo: once, before the first batch; the results then carry DQ in denovo_lr (pm_engine_set_vcf_denovo)
  virtual void set_vcf_denovo(bool on) { (void)on; throw FatalError("--vcf_denovo is not supported by this evaluator\n"); }
  // --vcf_denovo_chrX: once, after set_vcf_denovo(true) and before the first batch (pm_engine_set_vcf_denovo_chrx)
  virtual void set_vcf_denovo_chrx(bool on) { (void)on; throw FatalError("--vcf_denovo_chrX is not supported by this evaluator\n"); }
  // --vcf_denovo_chrX_detail: once, after set_vcf_denovo_chrx(true) and set_vcf_denovo_detail and before the first batch
  // (pm_engine_set_vcf_denovo_chrx_detail); vcf_denovo_rows and the two readers then serve chrX batches too
  virtual void set_vcf_denovo_chrx_detail(bool on) { (void)on; throw FatalError("--vcf_denovo_chrX_detail is not supported by this evaluator\n"); }
  // --vcf_denovo_families / --vcf_denovo_carriers: set_vcf_denovo_detail once, after set_vcf_denovo(true) and before the
  // first batch; then, for the batch the last run_vcf() returned (also after it threw a BrentError: the rows before the
  // stuck site), vcf_denovo_rows returns the row count and writes the rows' batch indices to site (may be null), and the
  // two readers hand out the rows [rows][K] (pm_engine_vcf_denovo_rows / _families / _carriers)
  virtual void set_vcf_denovo_detail(int fam_k, int car_k) {
    (void)fam_k; (void)car_k;
    throw FatalError("--vcf_denovo_families / --vcf_denovo_carriers is not supported by this evaluator\n");
  }
  virtual int vcf_denovo_rows(int32_t* site) {
    (void)site;
    throw FatalError("--vcf_denovo_families / --vcf_denovo_carriers is not supported by this evaluator\n");
  }
  virtual void vcf_denovo_families(pm_fam_lr* top) { (void)top; throw FatalError("--vcf_denovo_families is not supported by this evaluator\n"); }
  virtual void vcf_denovo_carriers(pm_person_dn* top) { (void)top; throw FatalError("--vcf_denovo_carriers is not supported by this evaluator\n"); }
  // --vcf_posteriors: set_vcf_posteriors once, before the first batch; then, for the batch the last run_vcf() returned
  // (also after it threw a BrentError: the rows it returned), vcf_posteriors writes the plane [rows][n_person] to out and
  // returns the row count (pm_engine_set_vcf_posteriors / pm_engine_vcf_posteriors)
  virtual void set_vcf_posteriors(bool on) { (void)on; throw FatalError("--vcf_posteriors is not supported by this evaluator\n"); }
  virtual int vcf_posteriors(pm_vcf_post* out) { (void)out; throw FatalError("--vcf_posteriors is not supported by this evaluator\n"); }
  // --vcf_phase: the same pair for the transmission phase plane (pm_engine_set_vcf_phase / pm_engine_vcf_phase)
  virtual void set_vcf_phase(bool on) { (void)on; throw FatalError("--vcf_phase is not supported by this evaluator\n"); }
  virtual int vcf_phase(pm_vcf_phase* out) { (void)out; throw FatalError("--vcf_phase is not supported by this evaluator\n"); }
  // --vcf_joint: the same pair for the joint call plane (pm_engine_set_vcf_joint / pm_engine_vcf_joint)
  virtual void set_vcf_joint(bool on) { (void)on; throw FatalError("--vcf_joint is not supported by this evaluator\n"); }
  virtual int vcf_joint(pm_vcf_joint* out) { (void)out; throw FatalError("--vcf_joint is not supported by this evaluator\n"); }
  // --vcf_pedcheck: set_vcf_pedcheck once, before the first batch; vcf_pedcheck, with no batch in flight, hands out the sums
  // over every batch so far, added over the evaluator's engines (pm_engine_set_vcf_pedcheck / pm_engine_vcf_pedcheck)
  virtual void set_vcf_pedcheck(bool on) { (void)on; throw FatalError("--vcf_pedcheck is not supported by this evaluator\n"); }
  virtual void vcf_pedcheck(std::vector<pm_vcf_pedcheck>& out) { (void)out; throw FatalError("--vcf_pedcheck is not supported by this evaluator\n"); }
  // Host memory for the batch buffers (the engine: page-locked, for asynchronous copies)
  virtual void* host_alloc(size_t bytes);
  virtual void host_free(void* p);

 private:
  std::vector<std::pair<int, int>> done_;   // (rows, first stuck site or -1) per submitted batch
};

// A run split over processes (one per GPU; polymutt_amd/launch.py): rank `rank` of `world` analyses a
// contiguous position range of every section.  `allgather` exchanges n int64 per rank (recv: world x n,
// rank-major); it is called the same number of times on every rank (once per section, once at the end).
struct ShardComm {
  int rank = 0, world = 1;
  std::function<void(const int64_t* send, int n, int64_t* recv)> allgather;
};

using EvaluatorFactory = std::function<std::unique_ptr<SiteEvaluator>(const pm_pedigree&, const pm_params&, const Options&)>;

int default_io_threads(const Options& opt);

// Runs the whole analysis; returns the process exit code.  With comm->world > 1 the run is one shard
// (run_polymutt_sharded).
int run_polymutt(const Options& opt, const Pedigree& ped, SiteEvaluator& eval, const ShardComm* comm = nullptr);

// The command line end to end (parse, pedigree, --glf2blocks, evaluator, run); FatalError -> the reference's
// "FATAL ERROR" text on stdout and exit code 1.
int polymutt_main(int argc, char** argv, const ShardComm* comm, const EvaluatorFactory& make);

}  // namespace pmhost
