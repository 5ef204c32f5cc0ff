// record_swap_plugin.cpp — NFCRecord::SwapRowInfo through NFGPUKernelModule
// (include/NFGPUKernelModule.hpp) from a game-server-style client: the script of
// tests/record_swap_model.py (the golden world of tests/golden/record_swap.json: REC / OBJ / INIT lines,
// then windows of SwapRowInfo calls among SetRecordObject / SetRecordInt / Remove / AddRow / ClearRecord
// calls with FindObject / FindInt / QueryRow / GetRecordObject calls between them, "X" the frame) is
// replayed through the plugin API, in the reference's logical columns.  The calls before a window's "X"
// see calls the library still holds queued (answered on the host), those after it the device's state.
// Every call line prints one line in the format of tests/cpp/record_swap_ref.cpp,
//   A <k> <ret> : <list>
// and every record event a frame delivers to the common record callback prints
//   E <window> <object> <record> <op> <row> <col> <old head> <old data> <new head> <new data>
// (op 0 Update, 1 Add, 2 Del, 3 Cover, 4 Swap with row the origin and col the target row; an int / f64
// value as head 0 and its bit pattern), which tests/test_gpu_record_swap.py compares with the recorded
// answers of the compiled reference, the events coalesced per window by the model's rule.
//
// usage: record_swap_plugin <script.txt>
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
static int g_window = 0;

struct RecDef {
    std::string name, types;
    int rows;
};

static NFGUID guid_of(const std::string& tok) {
    const size_t c = tok.find(':');
    return NFGUID(strtoll(tok.substr(0, c).c_str(), nullptr, 10), strtoll(tok.c_str() + c + 1, nullptr, 10));
}

static TData value_of(char type, const std::string& tok) {
    TData t;
    if (type == 'I') {
        t.type = TDATA_INT;
        t.i = strtoll(tok.c_str(), nullptr, 10);
    } else if (type == 'F') {
        t.type = TDATA_FLOAT;
        t.f = strtod(tok.c_str(), nullptr);
    } else {
        t.type = TDATA_OBJECT;
        t.o = guid_of(tok);
    }
    return t;
}

static void print_value(const TData& v) {
    unsigned long long h = 0, d = 0;
    if (v.type == TDATA_OBJECT) {
        h = (unsigned long long)v.o.nHead64;
        d = (unsigned long long)v.o.nData64;
    } else if (v.type == TDATA_INT) {
        d = (unsigned long long)v.i;
    } else if (v.type == TDATA_FLOAT) {
        memcpy(&d, &v.f, 8);
    }
    printf(" %llu %llu", h, d);
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
    std::map<std::string, int> rec_of;
    for (auto& d : defs) {
        std::vector<TDATA_TYPE> t;
        for (char c : d.types) t.push_back(c == 'I' ? TDATA_INT : c == 'F' ? TDATA_FLOAT : TDATA_OBJECT);
        rec_of[d.name] = km.AddRecord(d.name, d.rows, t);
        km.SetRecordFlags("Player", d.name, false, true, false);
    }
    km.Init();
    km.CreateScene(1);
    auto guid = [&](int o) { return NFGUID(7, 100 + o); };  // (o = n_obj: an NFGUID nobody has)
    auto rname = [&](int r) { return r >= 0 && r < (int)defs.size() ? defs[r].name : std::string("NoSuchRecord"); };
    for (int o = 0; o < n_obj; o++)
        if (!km.CreateObject(guid(o), 1, 1 + o % 3, "Player")) return 3;
    // the creation-time rows: cells [physical cols][rows] in row order (an NFGUID as its data word, then
    // its head word) and the used-row mask per (object, record)
    std::map<std::pair<int, int>, std::pair<uint64_t, std::vector<uint64_t>>> init;
    size_t at = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        if (f[0] == "REC" || f[0] == "OBJ") continue;
        if (f[0] != "INIT") break;
        const int o = atoi(f[1].c_str()), r = atoi(f[2].c_str()), row = atoi(f[3].c_str());
        size_t pcols = 0;
        for (char c : defs[r].types) pcols += c == 'O' ? 2 : 1;
        auto& st = init[{o, r}];
        st.second.resize(pcols * (size_t)defs[r].rows, 0);
        st.first |= 1ull << row;
        size_t p = 0;
        for (size_t c = 0; c < defs[r].types.size(); c++) {
            const TData v = value_of(defs[r].types[c], f[4 + c]);
            if (v.type == TDATA_OBJECT) {
                st.second[p++ * (size_t)defs[r].rows + row] = (uint64_t)v.o.nData64;
                st.second[p++ * (size_t)defs[r].rows + row] = (uint64_t)v.o.nHead64;
                continue;
            }
            uint64_t b = (uint64_t)v.i;
            if (v.type == TDATA_FLOAT) memcpy(&b, &v.f, 8);
            st.second[p++ * (size_t)defs[r].rows + row] = b;
        }
        printf("A %d %d :\n", (int)(at - defs.size() - 1), row);  // (a creation-time row: AddRow's return)
    }
    const int k0 = (int)(at - defs.size() - 1);
    for (auto& kv : init)
        if (!km.SetCreationRecord(guid(kv.first.first), defs[kv.first.second].name, kv.second.first, kv.second.second))
            return 3;
    km.RegisterCommonRecordEvent([&](const NFGUID& self, const RECORD_EVENT_DATA& e, const TData& o, const TData& n) {
        const int op = e.nOpType == RECORD_EVENT_DATA::Update ? 0 : e.nOpType == RECORD_EVENT_DATA::Add ? 1
                     : e.nOpType == RECORD_EVENT_DATA::Del  ? 2 : e.nOpType == RECORD_EVENT_DATA::Swap ? 4 : 3;
        printf("E %d %d %d %d %d %d", g_window, (int)(self.nData64 - 100), rec_of[e.strRecordName], op, e.nRow, e.nCol);
        print_value(o);
        print_value(n);
        printf("\n");
        return 0;
    });
    km.AfterInit();

    std::vector<int> last;
    int k = k0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        const std::string& op = f[0];
        if (op == "X") {
            g_now += 100;
            km.Execute();
            g_window++;
            continue;
        }
        const int o = atoi(f[1].c_str()), r = atoi(f[2].c_str());
        const NFGUID g = guid(o);
        const std::string rn = rname(r);
        const bool rknown = r >= 0 && r < (int)defs.size();
        long long ret = 0;
        std::vector<unsigned long long> lst;
        if (op == "AR") {
            std::vector<TData> v;
            for (size_t c = 0; rknown && c + 4 < f.size() && c < defs[r].types.size(); c++)
                v.push_back(value_of(defs[r].types[c], f[4 + c]));
            ret = km.AddRow(g, rn, atoi(f[3].c_str()), v);
        } else if (op == "SO") {
            ret = km.SetRecordObject(g, rn, atoi(f[3].c_str()), atoi(f[4].c_str()), guid_of(f[5]));
        } else if (op == "SI") {
            ret = km.SetRecordInt(g, rn, atoi(f[3].c_str()), atoi(f[4].c_str()), strtoll(f[5].c_str(), nullptr, 10));
        } else if (op == "RM") {
            ret = km.RemoveRow(g, rn, atoi(f[3].c_str()));
        } else if (op == "CL") {
            ret = km.ClearRecord(g, rn);
        } else if (op == "SW") {
            ret = km.SwapRowInfo(g, rn, atoi(f[3].c_str()), atoi(f[4].c_str()));
        } else if (op == "QR") {
            std::vector<TData> row;
            ret = km.QueryRow(g, rn, atoi(f[3].c_str()), row) ? 1 : 0;
            for (size_t c = 0; ret && c < row.size(); c++) {
                if (row[c].type == TDATA_OBJECT) {
                    lst.push_back((unsigned long long)row[c].o.nHead64);
                    lst.push_back((unsigned long long)row[c].o.nData64);
                    continue;
                }
                uint64_t b = (uint64_t)row[c].i;
                if (row[c].type == TDATA_FLOAT) memcpy(&b, &row[c].f, 8);
                lst.push_back(b);
            }
        } else if (op == "GO") {
            const NFGUID v = km.GetRecordObject(g, rn, atoi(f[3].c_str()), atoi(f[4].c_str()));
            lst.push_back((unsigned long long)v.nHead64);
            lst.push_back((unsigned long long)v.nData64);
        } else if (op[0] == 'F') {
            if (op.back() != '+') last.clear();
            const int col = atoi(f[3].c_str());
            if (op[1] == 'O') {
                ret = km.FindObject(g, rn, col, guid_of(f[4]), last);
            } else {
                ret = km.FindInt(g, rn, col, strtoll(f[4].c_str(), nullptr, 10), last);
            }
            for (int x : last) lst.push_back((unsigned long long)x);
        } else {
            fprintf(stderr, "bad script line %zu\n", at);
            return 2;
        }
        printf("A %d %lld :", k++, ret);
        for (unsigned long long x : lst) printf(" %llu", x);
        printf("\n");
    }
    km.BeforeShut();
    km.Shut();
    return 0;
}
