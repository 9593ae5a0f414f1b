// geglove -c <config.yml> : the reference's CLI (J/Main.java:133-160) over the MI355X library.
// Same single flag, same settings banner, same output files ./out/<name>.{vectors,dict}.tsv
// (and <name>.neighbors.tsv with `device: { neighbors: K }`, <name>.holdout.tsv with `device: { holdout: F }`,
// <name>.rank.tsv with `device: { rank: Q }`, <name>.clusters.tsv with `device: { clusters: K }`,
// <name>.links.tsv with `device: { predict: K }`, <name>.foldin.tsv with `device: { foldin: F }`,
// <name>.classes.tsv with `device: { classify: labels.tsv }`,
// <name>.matches.tsv and <name>.entities.tsv with `device: { match: T }`,
// <name>.alignment.tsv with `device: { align: T, align_source: P, align_target: Q }`).
#include <ctime>
#include "ge_host.hpp"

using namespace ge_host;

static void log_info(const std::string &who, const std::string &msg) {      // log4j pattern %d{HH:mm:ss} %-5p %-25c{1} :: %m%n
    char ts[16];
    const std::time_t t = std::time(nullptr);
    std::strftime(ts, sizeof ts, "%H:%M:%S", std::localtime(&t));
    std::printf("%s %-5s %-25s :: %s\n", ts, "INFO", who.c_str(), msg.c_str());
    std::fflush(stdout);
}
static void log_warn(const std::string &who, const std::string &msg) {
    char ts[16];
    const std::time_t t = std::time(nullptr);
    std::strftime(ts, sizeof ts, "%H:%M:%S", std::localtime(&t));
    std::printf("%s %-5s %-25s :: %s\n", ts, "WARN", who.c_str(), msg.c_str());
    std::fflush(stdout);
}
static void log_error(const std::string &msg) {
    char ts[16];
    const std::time_t t = std::time(nullptr);
    std::strftime(ts, sizeof ts, "%H:%M:%S", std::localtime(&t));
    std::fprintf(stderr, "%s %-5s %-25s :: %s\n", ts, "ERROR", "Graph Embeddings", msg.c_str());
}
static double g_tolerance = 0;
static const IOptimizer *g_optimizer = nullptr;          // the run's optimizer, for the held-out cost beside the training cost
static void progress(int iteration, double cost, double diff) {
    char b[200];
    const double held = g_optimizer ? g_optimizer->lastHoldoutCost() : std::nan("");
    if (held == held) std::snprintf(b, sizeof b, "epoch %d  cost %.9g  holdout %.9g  %.6g/%.6g", iteration + 1, cost, held, diff, g_tolerance);
    else std::snprintf(b, sizeof b, "epoch %d  cost %.9g  %.6g/%.6g", iteration + 1, cost, diff, g_tolerance);
    log_info("Optimizer", b);
}

static void runProgram(const Configuration &given) {                        // J/Main.java:29-78
    Configuration config = given;               // `device.holdout` pins the seed and learns the split's counts below
    for (auto &l : config.banner()) log_info("Graph Embeddings", l);
    for (auto &k : config.ignored_keys) log_info("Configuration", "ignoring key not known to this revision's bean: " + k);
    std::string outFileName = config.output.name;
    if (outFileName.empty()) outFileName = createFileName(config);
    log_info("Graph Embeddings", "Writing files with prefix: " + outFileName);

    std::unique_ptr<InMemoryGraph> graph;
    std::unique_ptr<CoOccurrenceMatrix> matrix;
    if (!config.device.load_coo.empty()) {
        matrix.reset(new StoredCooMatrix(config.device.load_coo));
        log_info("BookmarkColoring", "loaded COO checkpoint " + config.device.load_coo);
    } else {
        if (!config.usingSimilarity()) log_info("Rdf2GrphConverter", "Partial matching is disabled, no edges between similar literals are added");
        graph.reset(new InMemoryGraph(read_ntriples(config.graph, config, true, config.device.id,
                                                    [](const std::string &m) { log_info("Rdf2GrphConverter", m); })));
        char b[200];
        std::snprintf(b, sizeof b, "Skipped %lld unweighted triples (%.2f %%)", graph->skipped,
                      graph->triples ? 100.0 * (double)graph->skipped / (double)graph->triples : 0.0);
        log_info("Rdf2GrphConverter", b);
        std::snprintf(b, sizeof b, "graph: %d vertices, %zu out-neighbour pairs", graph->V, graph->out_idx.size());
        log_info("Rdf2GrphConverter", b);
        if (config.device.gpus > 1) matrix.reset(new ShardedBookmarkColoring(*graph, config));
        else matrix.reset(new BookmarkColoring(*graph, config));
        if (!config.device.save_coo.empty()) {
            StoredCooMatrix::save(config.device.save_coo, *matrix);
            log_info("BookmarkColoring", "wrote COO checkpoint " + config.device.save_coo);
        }
    }
    {
        char b[200];
        std::snprintf(b, sizeof b, "BCA: %d co-occurrences, max %.9g", matrix->coOccurrenceCount(), matrix->max());
        log_info("BookmarkColoring", b);
    }
    std::unique_ptr<HoldoutMatrix> split;
    if (config.holdingOut()) {
        config.device.seed = config.runSeed(); config.device.has_seed = true;      // one seed for the split and the trainer
        split.reset(new HoldoutMatrix(*matrix, (uint64_t)config.device.seed, config.device.holdout));
        config.device.holdout_held = split->heldCount(); config.device.holdout_total = matrix->coOccurrenceCount();
        log_info("Graph Embeddings", config.banner().back());
    }
    std::unique_ptr<FoldinMatrix> late;
    if (config.foldingIn()) {
        config.device.seed = config.runSeed(); config.device.has_seed = true;      // one seed for the split, the trainer and the fold-in's walk
        late.reset(new FoldinMatrix(*matrix, (uint64_t)config.device.seed, config.device.foldin));
        config.device.foldin_late = (long long)late->lateVertices().size(); config.device.foldin_vertices = matrix->vocabSize();
        log_info("Graph Embeddings", config.banner().back());
    }
    const CoOccurrenceMatrix &bca = split ? static_cast<const CoOccurrenceMatrix &>(*split) : late ? static_cast<const CoOccurrenceMatrix &>(*late) : *matrix;
    g_tolerance = config.opt.tolerance;
    std::unique_ptr<IOptimizer> optimizer = createOptimizer(config, bca, progress);
    if (split) { optimizer->holdOut(split->heldI(), split->heldJ(), split->heldX(), split->heldCount()); g_optimizer = optimizer.get(); }
    if (!optimizer->scheduleNote().empty()) log_info("Optimizer", optimizer->scheduleNote());
    Optimum optimum = optimizer->optimize();
    if (late)                                   // the late vertices get their focus rows before anything reads the tables
        optimizer->foldIn(late->lateVertices(), late->latePtr(), late->lateIdx(), late->lateX(), (int32_t)config.device.foldin_epochs,
                          (int64_t)config.device.seed, optimum);
    if (split && config.ranking()) {            // on the tables as the last epoch left them
        std::vector<int32_t> rI, rJ, fIdx; std::vector<int64_t> fPtr;
        split->rankSet(config.device.rank, rI, rJ, fPtr, fIdx);
        optimizer->rank(rI, rJ, fPtr, fIdx, optimum);
    }
    if (config.predicting()) {                  // likewise, while the handle lives
        std::vector<int32_t> pI, fIdx; std::vector<int64_t> fPtr;
        predictSet(config, bca, pI, fPtr, fIdx);
        if (!pI.empty()) optimizer->predict(pI, fPtr, fIdx, pI, (int32_t)config.device.predict, optimum);
    }
    {
        char b[120];
        std::snprintf(b, sizeof b, "Finished optimization with final cost: %.12g", optimum.finalCost);
        log_info("Optimizer", b);
    }
    if (config.applyingPca()) log_info("PCA", applyPca(config, optimum, bca.vocabSize()));
    EmbeddingTextWriter writer(outFileName, config);
    const long long n = writer.write(optimum, bca, "out");
    log_info("EmbeddingTextWriter", "wrote " + std::to_string(n) + " vectors to out/" + writer.vectorsFile());
    if (split) log_info("Holdout", writeHoldout(config, optimum, outFileName, "out"));
    if (late) log_info("Foldin", writeFoldin(config, optimum, bca, outFileName, "out"));
    if (split && config.ranking()) log_info("Rank", writeRank(config, optimum, outFileName, "out"));
    if (config.predicting()) log_info("Predict", writeLinks(config, optimum, bca, outFileName, "out"));
    if (config.writingNeighbors()) {
        std::string warning;
        const std::string done = writeNeighbors(config, optimum, bca, outFileName, "out", warning);
        if (!warning.empty()) log_warn("Neighbors", warning);
        log_info("Neighbors", done);
    }
    if (config.clustering()) {
        std::string warning;
        const std::string done = writeClusters(config, optimum, bca, outFileName, "out", (uint64_t)config.runSeed(), warning);
        if (!warning.empty()) log_warn("Clusters", warning);
        log_info("Clusters", done);
    }
    if (config.classifying()) {
        std::string warning;
        const std::string done = writeClasses(config, optimum, bca, outFileName, "out", (uint64_t)config.runSeed(), warning);
        if (!warning.empty()) log_warn("Classify", warning);
        log_info("Classify", done);
    }
    if (config.matching()) log_info("Match", writeMatches(config, optimum, bca, outFileName, "out"));
    if (config.aligning()) log_info("Align", writeAlignment(config, optimum, bca, outFileName, "out"));
    g_optimizer = nullptr;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        if (std::string(argv[i]) == "-c") {
            if (i + 1 < argc) {
                try {
                    std::ifstream probe(argv[i + 1]);
                    if (!probe) { log_error(std::string("Cannot find configuration file + ") + argv[i + 1]); return 1; }
                    probe.close();
                    const Configuration config = Configuration::load(argv[i + 1]);
                    Configuration::check(config);
                    runProgram(config);
                } catch (const std::exception &e) {
                    log_error(e.what());
                    return 1;
                }
            } else {
                log_error("No configuration file specified, exiting...");
                return 1;
            }
        }
    }
    return 0;
}
