// record_find_plugin.cpp — the record finds of NFGPUKernelModule (include/NFGPUKernelModule.hpp) from a
// game-server-style client: the script of tests/record_find_model.py (the golden world of
// tests/golden/record_find.json: REC / OBJ / INIT lines, then windows of SetRecordInt / Remove / AddRow /
// ClearRecord calls with FindInt / FindFloat / FindRowByColValue / QueryRow calls between them, "X" the
// frame) is replayed through the plugin API.  The finds before a window's "X" see calls the library
// still holds queued (answered on the host), the finds after it the device's state.  Every find /
// QueryRow prints one line in the format of tests/cpp/record_find_ref.cpp,
//   A <k> <ret> : <rows of varResult>          (QR: <0 | 1> : the row's cells as uint64 bit patterns)
// which tests/test_gpu_record_find.py compares with the recorded answers of the compiled reference.
//
// usage: record_find_plugin <script.txt>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "NFGPUKernelModule.hpp"

using namespace nfgpu;

static int64_t g_now = 0;

struct RecDef {
    std::string name, types;
    int rows;
};

static TData value_of(char type, const std::string& tok) {
    TData t;
    if (type == 'I') {
        t.type = TDATA_INT;
        t.i = strtoll(tok.c_str(), nullptr, 10);
    } else {
        t.type = TDATA_FLOAT;
        t.f = strtod(tok.c_str(), nullptr);
    }
    return t;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::vector<std::vector<std::string>> lines;
    for (std::string ln; std::getline(in, ln);) {
        std::istringstream ss(ln);
        std::vector<std::string> f;
        for (std::string t; ss >> t;) f.push_back(t);
        if (!f.empty()) lines.push_back(f);
    }
    std::vector<RecDef> defs;
    int n_obj = 0;
    for (auto& f : lines) {
        if (f[0] == "REC") defs.push_back({f[1], f[3], atoi(f[2].c_str())});
        if (f[0] == "OBJ") n_obj = atoi(f[1].c_str());
    }
    NFGPUKernelModule km(n_obj + 8);
    km.SetTimeSource([] { return g_now; });
    km.AddProperty("HP", TDATA_INT);
    km.AddClass("Player");
    km.SetPropertyFlags("Player", "HP", false, true, false);
    for (auto& d : defs) {
        std::vector<TDATA_TYPE> t;
        for (char c : d.types) t.push_back(c == 'I' ? TDATA_INT : TDATA_FLOAT);
        km.AddRecord(d.name, d.rows, t);
        km.SetRecordFlags("Player", d.name, false, true, false);
    }
    km.Init();
    km.CreateScene(1);
    auto guid = [&](int o) { return NFGUID(7, 100 + o); };  // (o = n_obj: an NFGUID nobody has)
    auto rname = [&](int r) { return r >= 0 && r < (int)defs.size() ? defs[r].name : std::string("NoSuchRecord"); };
    for (int o = 0; o < n_obj; o++)
        if (!km.CreateObject(guid(o), 1, 1 + o % 3, "Player")) return 3;
    // the creation-time rows: cells [cols][rows] in row order and the used-row mask per (object, record)
    std::map<std::pair<int, int>, std::pair<uint64_t, std::vector<uint64_t>>> init;
    size_t at = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        if (f[0] == "REC" || f[0] == "OBJ") continue;
        if (f[0] != "INIT") break;
        const int o = atoi(f[1].c_str()), r = atoi(f[2].c_str()), row = atoi(f[3].c_str());
        auto& st = init[{o, r}];
        st.second.resize(defs[r].types.size() * (size_t)defs[r].rows, 0);
        st.first |= 1ull << row;
        for (size_t c = 0; c < defs[r].types.size(); c++) {
            const TData v = value_of(defs[r].types[c], f[4 + c]);
            uint64_t b = (uint64_t)v.i;
            if (v.type == TDATA_FLOAT) memcpy(&b, &v.f, 8);
            st.second[c * (size_t)defs[r].rows + row] = b;
        }
    }
    for (auto& kv : init)
        if (!km.SetCreationRecord(guid(kv.first.first), defs[kv.first.second].name, kv.second.first, kv.second.second))
            return 3;
    km.AfterInit();

    std::vector<int> last;
    int k = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        const std::string& op = f[0];
        if (op == "X") {
            g_now += 100;
            km.Execute();
            continue;
        }
        const int o = atoi(f[1].c_str()), r = atoi(f[2].c_str());
        const NFGUID g = guid(o);
        const std::string rn = rname(r);
        if (op == "AR") {
            std::vector<TData> v;
            for (size_t c = 0; c + 4 < f.size(); c++) v.push_back(value_of(defs[r].types[c], f[4 + c]));
            km.AddRow(g, rn, atoi(f[3].c_str()), v);
        } else if (op == "SI") {
            km.SetRecordInt(g, rn, atoi(f[3].c_str()), atoi(f[4].c_str()), strtoll(f[5].c_str(), nullptr, 10));
        } else if (op == "RM") {
            km.RemoveRow(g, rn, atoi(f[3].c_str()));
        } else if (op == "CL") {
            km.ClearRecord(g, rn);
        } else if (op == "QR") {
            std::vector<TData> row;
            const bool ok = km.QueryRow(g, rn, atoi(f[3].c_str()), row);
            printf("A %d %d :", k++, ok ? 1 : 0);
            for (size_t c = 0; ok && c < row.size(); c++) {
                uint64_t b = (uint64_t)row[c].i;
                if (row[c].type == TDATA_FLOAT) memcpy(&b, &row[c].f, 8);
                printf(" %llu", (unsigned long long)b);
            }
            printf("\n");
        } else if (op[0] == 'F') {
            if (op.back() != '+') last.clear();
            const int col = atoi(f[3].c_str());
            int ret;
            if (op[1] == 'I') {
                ret = km.FindInt(g, rn, col, strtoll(f[4].c_str(), nullptr, 10), last);
            } else if (op[1] == 'F') {
                ret = km.FindFloat(g, rn, col, strtod(f[4].c_str(), nullptr), last);
            } else {
                std::vector<TData> var;
                for (int e = 0; e < atoi(f[4].c_str()); e++) var.push_back(value_of(f[5 + 2 * e][0], f[6 + 2 * e]));
                ret = km.FindRowByColValue(g, rn, col, var, last);
            }
            printf("A %d %d :", k++, ret);
            for (int x : last) printf(" %d", x);
            printf("\n");
        } else {
            fprintf(stderr, "bad script line %zu\n", at);
            return 2;
        }
    }
    km.BeforeShut();
    km.Shut();
    return 0;
}
