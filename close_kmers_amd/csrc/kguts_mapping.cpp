/*
 * kguts_mapping.cpp -- the facade's family data base and what reads it:
 * KmerPegMapping (kmer_to_id_ / kmer_to_family_id_ on the device, the genus
 * and family tables on the host), MatrixRequest and FamilyMapper
 * (family_mapper.cc:46-205, 287-330).
 */
#include "kguts_impl.h"

#include <fstream>
#include <iostream>

namespace kgx {

/* ---- KmerPegMapping / MatrixRequest ------------------------------------ */

KmerPegMapping::KmerPegMapping(int device) : device_(device)
{
    int rc = kgx_kmap_create(device, KGX_KMAP_APPEND, &kmer_to_id_);
    if (!rc)
        rc = kgx_kmap_create(device, KGX_KMAP_SET, &kmer_to_family_id_);
    if (rc) {
        kgx_kmap_destroy(kmer_to_id_);
        throw_last(rc, "kgx_kmap_create");
    }
}

KmerPegMapping::~KmerPegMapping()
{
    kgx_kmap_destroy(kmer_to_id_);
    kgx_kmap_destroy(kmer_to_family_id_);
}

KmerPegMapping::encoded_id_t KmerPegMapping::encode_id(const std::string &peg)
{
    auto it = peg_to_id_.find(peg);
    if (it != peg_to_id_.end())
        return it->second;
    const encoded_id_t id = (encoded_id_t)id_to_peg_.size();
    peg_to_id_[peg] = id;
    id_to_peg_.push_back(peg);
    return id;
}

std::string KmerPegMapping::lookup_genus(const std::string &genus)
{
    std::lock_guard<std::mutex> lk(genus_mu_);
    return genus_map_[genus];
}

bool KmerPegMapping::find_genus(const std::string &genus, std::string *id) const
{
    std::lock_guard<std::mutex> lk(genus_mu_);
    auto it = genus_map_.find(genus);
    if (it == genus_map_.end())
        return false;
    *id = it->second;
    return true;
}

KmerPegMapping::family_data_t KmerPegMapping::family_at(encoded_family_id_t id) const
{
    auto it = family_data_.find(id);
    return it == family_data_.end() ? family_data_t{} : it->second;
}

std::string KmerPegMapping::decode_id(encoded_id_t id) const
{
    return id < id_to_peg_.size() ? id_to_peg_[id] : std::string();
}

void KmerPegMapping::dump_sizes(std::ostream &os) const
{
    os << "kmer_to_id_: size=" << kgx_kmap_num_kmers(kmer_to_id_) << "\n";
    os << "kmer_to_id_: content size=" << kgx_kmap_num_values(kmer_to_id_) << "\n";
    os << "peg_to_id_: size=" << peg_to_id_.size() << "\n";
    os << "id_to_peg_: size=" << id_to_peg_.size() << "\n";
    os << "genome_to_id_: size=0\n";
    os << "id_to_genome_: size=0\n";
}

void KmerPegMapping::add_batch_mappings(KmerGuts &kg, const std::vector<encoded_id_t> &ids)
{
    int rc = kgx_kmap_add_hits(kmer_to_id_, kg.ctx(), ids.data());
    if (rc)
        throw_last(rc, "kgx_kmap_add_hits");
}

void KmerPegMapping::add_batch_fam_mappings(KmerGuts &kg, const std::vector<encoded_family_id_t> &ids)
{
    int rc = kgx_kmap_add_hits(kmer_to_family_id_, kg.ctx(), ids.data());
    if (rc)
        throw_last(rc, "kgx_kmap_add_hits");
}

MatrixRequest::MatrixRequest(std::shared_ptr<KmerPegMapping> mapping) : mapping_(mapping)
{
    int rc = kgx_matrix_create(mapping_->kmer_to_id(), &mx_);
    if (rc)
        throw_last(rc, "kgx_matrix_create");
}

MatrixRequest::~MatrixRequest() { kgx_matrix_destroy(mx_); }

void MatrixRequest::process_work(KmerGuts &kg, const std::vector<std::pair<std::string, std::string>> &work)
{
    std::vector<KmerPegMapping::encoded_id_t> ids;
    std::vector<std::string> seqs;
    for (auto &w : work) {
        const KmerPegMapping::encoded_id_t eid = mapping_->encode_id(w.first);
        matrix_proteins_[eid] = w.second.size(); /* matrix_request.cc:91 */
        ids.push_back(eid);
        seqs.push_back(w.second);
    }
    run_batch_on_device(kg, seqs);
    int rc = kgx_matrix_add_hits(mx_, kg.ctx(), ids.data());
    if (rc)
        throw_last(rc, "kgx_matrix_add_hits");
}

void MatrixRequest::write_results(std::ostream &os)
{
    const kgx_pair_count *p = nullptr;
    uint64_t n = 0;
    int rc = kgx_matrix_pairs(mx_, &p, &n);
    if (rc)
        throw_last(rc, "kgx_matrix_pairs");
    for (uint64_t i = 0; i < n; i++) {
        const size_t l1 = matrix_proteins_[p[i].id1], l2 = matrix_proteins_[p[i].id2];
        const float score = (float)p[i].count / ((float)(l1 + l2));
        os << mapping_->decode_id(p[i].id1) << "\t" << mapping_->decode_id(p[i].id2) << "\t"
           << (unsigned long)p[i].count << "\t" << score << "\n";
    }
}

/* ---- family DB, FamilyMapper --------------------------------------------- */

KmerPegMapping::encoded_id_t KmerPegMapping::assign_new_peg_id(const std::string &peg)
{
    const encoded_id_t id = (encoded_id_t)id_to_peg_.size();
    peg_to_id_[peg] = id;
    id_to_peg_.push_back(peg);
    return id;
}

static std::vector<std::string> split_tabs(const std::string &line)
{
    std::vector<std::string> cols; /* boost::split(cols, line, is_any_of("\t")) */
    size_t a = 0;
    for (;;) {
        size_t b = line.find('\t', a);
        cols.push_back(line.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos)
            return cols;
        a = b + 1;
    }
}

void KmerPegMapping::load_genus_map(const std::string &genus_file)
{
    std::ifstream gf(genus_file);
    if (gf.fail())
        throw Error(KGX_EIO, "Error opening gnus file " + genus_file);
    std::string line;
    while (std::getline(gf, line)) {
        auto cols = split_tabs(line);
        genus_map_[cols[0]] = cols.size() > 1 ? cols[1] : std::string();
    }
}

void KmerPegMapping::load_families(const std::string &families_file)
{
    std::ifstream f(families_file);
    if (f.fail())
        throw Error(KGX_EIO, "Failure opening families file " + families_file);
    const std::string zeros("00000000");
    std::string line;
    while (std::getline(f, line)) {
        auto cols = split_tabs(line);
        if (cols.size() < 9)
            continue;
        std::string pgf = "PGF_" + cols[0].substr(2);
        std::string plf("PLF_");
        unsigned long genus_id = 0;
        auto mapped = genus_map_.find(cols[7]);
        if (mapped == genus_map_.end()) {
            plf += cols[7];
        } else {
            plf += mapped->second;
            genus_id = std::stoul(mapped->second);
        }
        plf += "_";
        plf += zeros.substr(0, 8 - cols[8].size());
        plf += cols[8];
        const encoded_id_t id = assign_new_peg_id(cols[3]);
        const unsigned long seqlen = std::stoul(cols[4]);
        auto fkey = std::make_pair(pgf, plf);
        encoded_family_id_t fam_id;
        auto fit = family_key_to_id_.find(fkey);
        if (fit == family_key_to_id_.end()) {
            fam_id = next_family_id_++;
            family_key_to_id_[fkey] = fam_id;
            family_data_.emplace(fam_id, family_data_t{pgf, plf, genus_id, cols[5], fam_id, seqlen, 1});
        } else {
            fam_id = fit->second;
            family_data_t &d = family_data_[fam_id];
            d.total_size += seqlen;
            d.count++;
        }
        peg_to_family_.insert(std::make_pair(id, fam_id));
    }
}

void KmerPegMapping::load_nr_families(KmerGuts &kg, const std::string &nr_fasta, size_t batch)
{
    std::ifstream in(nr_fasta, std::ios::binary);
    if (!in)
        throw Error(KGX_EIO, "cannot open " + nr_fasta);
    std::vector<std::string> seqs;
    std::vector<encoded_family_id_t> fams;
    auto flush = [&]() {
        if (seqs.empty())
            return;
        run_batch_on_device(kg, seqs);
        add_batch_fam_mappings(kg, fams);
        seqs.clear();
        fams.clear();
    };
    FastaParser parser;
    parser.set_callback([&](const std::string &id, const std::string &seq) {
        auto fit = peg_to_family_.find(encode_id(id));
        if (fit == peg_to_family_.end())
            return 0; /* "NO FAM FOR id=..." (nr_loader.cc:150-156) */
        seqs.push_back(seq);
        fams.push_back(fit->second);
        if (seqs.size() >= batch)
            flush();
        return 0;
    });
    char ch;
    while (in.get(ch))
        parser.parse_char(ch);
    parser.parse_complete();
    flush();
}

FamilyMapper::FamilyMapper(KmerGuts &kg, std::shared_ptr<KmerPegMapping> mapping) : kg_(kg), mapping_(mapping) {}

FamilyMapper::best_match_t FamilyMapper::find_best_family_match(const kgx_rollup_row *rows, size_t n_rows,
                                                                 std::vector<KmerCall> &calls)
{
    int fi;
    std::string fn;
    float score, wscore, off = 0.0f;
    kg_.find_best_call(calls, fi, fn, score, wscore, off);
    return match_from(rows, n_rows, fn, score);
}

FamilyMapper::best_match_t FamilyMapper::find_best_family_match(const kgx_rollup_row *rows, size_t n_rows,
                                                                 const kgx_best_call &best)
{
    int fi;
    std::string fn;
    float score, wscore, off = 0.0f;
    kg_.find_best_call(best, fi, fn, score, wscore, off);
    return match_from(rows, n_rows, fn, score);
}

FamilyMapper::best_match_t FamilyMapper::match_from(const kgx_rollup_row *rows, size_t n_rows, std::string fn,
                                                    float score)
{
    /* ingest_protein clears seq_score_ (family_mapper.cc:48); on_hit's
     * operator[] calls (family_mapper.cc:287-312) leave the ids in
     * first-touch order, which is the rows' order */
    seq_score_.clear();
    fill_scores(seq_score_, rows, n_rows);
    if (fn.empty() || fn.find(" ?? ") != std::string::npos)
        fn = "hypothetical protein"; /* allow_ambiguous_functions_ = false */
    float best_lf = 0.0f, best_gf = 0.0f;
    std::string lf, gf;
    std::unordered_map<std::string, float> pgf_rollup;
    for (auto hit_ent : seq_score_) {
        const sequence_accumulated_score_t &se = hit_ent.second;
        if (se.hit_total < kmer_hit_threshold_)
            continue;
        auto fent = mapping_->family_data_.find(hit_ent.first);
        if (fent == mapping_->family_data_.end())
            continue;
        const KmerPegMapping::family_data_t &fd = fent->second;
        if (fd.function != fn)
            continue;
        pgf_rollup[fd.pgf] += se.weighted_total;
        if (se.weighted_total > best_lf) {
            best_lf = se.weighted_total;
            lf = fd.plf;
        }
    }
    for (auto pgf_ent : pgf_rollup)
        if (pgf_ent.second > best_gf) {
            best_gf = pgf_ent.second;
            gf = pgf_ent.first;
        }
    return best_match_t{gf, best_gf, lf, best_lf, fn, score};
}

std::ostream &operator<<(std::ostream &os, const FamilyMapper::best_match_t &m)
{
    /* family_mapper.h:70-75 */
    os << m.gfam_id << "\t" << m.gfam_score << "\t" << m.lfam_id << "\t" << m.lfam_score << "\t" << m.function
       << "\t" << m.score;
    return os;
}

}  // namespace kgx
