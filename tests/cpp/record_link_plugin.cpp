// record_link_plugin.cpp — property links through NFGPUKernelModule::LinkRecordColumns
// (include/NFGPUKernelModule.hpp) from a game-server-style client: the script of
// tests/record_link_model.py (the golden world of tests/golden/record_link.json; the line formats are in
// tests/cpp/record_link_ref.cpp) replayed through the plugin API.  The Player's CommPropertyValue record
// is linked over all its rows, a column to the property its tag names (none for a tag that starts with
// '_'); an object starts as the reference's module leaves it after CreateObject: every row used, row 0
// the BASE values, every linked property its base value.  The module's calls are made as a client makes
// them: SV a SetRecordInt on the group's row, AV / UV a GetRecordInt and a SetRecordInt, LV (the level
// callback's RefreshBaseProperty) one SetRecordInt on row 0 per column, in column order.  One more line,
//   SP <o> <name> <v>                   SetPropertyInt (false and nothing queued on a linked name)
// Every call line prints, in record_link_ref.cpp's format,
//   A <k> <ret> : <GetPropertyInt of every tag's property of object o, in column order (0 for none)>
// (the values as the reference holds them right after the call: the window's queued calls replayed),
// and every property event a frame ("X") delivers to the common property callback
//   P <window> <object> <name> <old> <new>
// and, first, "R refused": LinkRecordColumns on a record with an object column throws.
//
// usage: record_link_plugin <script.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "NFGPUKernelModule.hpp"

using namespace nfgpu;

static int64_t g_now = 0;
static int g_window = 0;

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
    int rows = 0, cols = 0, n_obj = 0;
    std::vector<std::string> tags, names;
    std::vector<long long> base;
    size_t at = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        if (f[0] == "SHAPE") {
            rows = atoi(f[1].c_str());
            cols = atoi(f[2].c_str());
        } else if (f[0] == "TAGS") {
            tags.assign(f.begin() + 1, f.end());
            for (auto& t : tags) names.push_back(t[0] == '_' ? std::string() : t);
        } else if (f[0] == "BASE") {
            for (size_t c = 1; c < f.size(); c++) base.push_back(strtoll(f[c].c_str(), nullptr, 10));
        } else if (f[0] == "OBJ") {
            n_obj = atoi(f[1].c_str());
        } else {
            break;
        }
    }
    if (rows <= 0 || (int)names.size() != cols || (int)base.size() != cols || n_obj <= 0) return 2;
    const int rows_l = rows;
    auto col_of = [&](const std::string& tag) {
        for (int c = 0; c < cols; c++)
            if (tags[(size_t)c] == tag) return c;
        return -1;
    };
    const std::string rec = "CommPropertyValue";
    {  // a record with an object column cannot be linked (a Swap's target names a physical column there)
        NFGPUKernelModule probe(8);
        probe.AddProperty("MAXHP", TDATA_INT);
        probe.AddRecord("Bag", 4, {TDATA_OBJECT, TDATA_INT});
        try {
            probe.LinkRecordColumns("Bag", 4, {"", "MAXHP"});
            printf("R linked\n");
        } catch (const std::invalid_argument&) {
            printf("R refused\n");
        }
    }
    NFGPUKernelModule km(n_obj + 8);
    km.SetTimeSource([] { return g_now; });
    km.AddClass("Player");
    km.AddProperty("Free", TDATA_INT);  // (an int property no column is linked to)
    km.SetPropertyFlags("Player", "Free", false, true, false);
    for (auto& nm : names)
        if (!nm.empty()) {
            km.AddProperty(nm, TDATA_INT);
            km.SetPropertyFlags("Player", nm, true, true, false);
        }
    km.AddRecord(rec, rows, std::vector<TDATA_TYPE>((size_t)cols, TDATA_INT));
    km.SetRecordFlags("Player", rec, false, true, false);
    km.LinkRecordColumns(rec, rows_l, names);
    km.Init();
    km.CreateScene(1);
    auto guid = [&](int o) { return NFGUID(7, 100 + o); };
    std::vector<uint64_t> cells((size_t)rows * cols, 0);  // [cols][rows]: row 0 the base values
    std::map<std::string, TData> init;
    for (int c = 0; c < cols; c++) {
        cells[(size_t)c * rows] = (uint64_t)base[(size_t)c];
        if (names[(size_t)c].empty()) continue;
        TData t;
        t.type = TDATA_INT;
        t.i = base[(size_t)c];
        init[names[(size_t)c]] = t;
    }
    for (int o = 0; o < n_obj; o++) {
        if (!km.CreateObject(guid(o), 1, 1 + o % 3, "Player", init)) return 3;
        if (!km.SetCreationRecord(guid(o), rec, (1ull << rows_l) - 1, cells)) return 3;
    }
    km.RegisterCommonPropertyEvent([&](const NFGUID& self, const std::string& name, const TData& o, const TData& n) {
        printf("P %d %d %s %lld %lld\n", g_window, (int)(self.nData64 - 100), name.c_str(), (long long)o.i, (long long)n.i);
        return 0;
    });
    km.AfterInit();

    int k = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        const std::string& op = f[0];
        if (op == "X") {
            g_now += 100;
            km.Execute();
            g_window++;
            continue;
        }
        const int o = atoi(f[1].c_str());
        const NFGUID g = guid(o);
        long long ret = 0;
        if (op == "SV" || op == "AV" || op == "UV") {
            const int row = atoi(f[2].c_str()), col = col_of(f[3]);
            int v = (int)strtoll(f[4].c_str(), nullptr, 10);
            if (op != "SV") {  // (the module's arithmetic is on ints)
                const int cur = (int)km.GetRecordInt(g, rec, row, col);
                v = op == "AV" ? cur + v : cur - v;
            }
            ret = km.SetRecordInt(g, rec, row, col, v);
        } else if (op == "LV") {
            ret = 1;
            for (int c = 0; c < cols; c++)
                ret = ret && km.SetRecordInt(g, rec, 0, c, (int)strtoll(f[3 + (size_t)c].c_str(), nullptr, 10));
        } else if (op == "SI") {
            ret = km.SetRecordInt(g, rec, atoi(f[2].c_str()), atoi(f[3].c_str()), strtoll(f[4].c_str(), nullptr, 10));
        } else if (op == "AR") {
            std::vector<TData> v;
            for (size_t c = 3; c < f.size(); c++) {
                TData t;
                t.type = TDATA_INT;
                t.i = strtoll(f[c].c_str(), nullptr, 10);
                v.push_back(t);
            }
            ret = km.AddRow(g, rec, atoi(f[2].c_str()), v);
        } else if (op == "RM") {
            ret = km.RemoveRow(g, rec, atoi(f[2].c_str()));
        } else if (op == "CL") {
            ret = km.ClearRecord(g, rec);
        } else if (op == "SW") {
            ret = km.SwapRowInfo(g, rec, atoi(f[2].c_str()), atoi(f[3].c_str()));
        } else if (op == "SP") {
            ret = km.SetPropertyInt(g, f[2], strtoll(f[3].c_str(), nullptr, 10));
        } else {
            fprintf(stderr, "bad script line %zu\n", at);
            return 2;
        }
        printf("A %d %lld :", k++, ret);
        for (auto& nm : names) printf(" %lld", nm.empty() ? 0ll : (long long)km.GetPropertyInt(g, nm));
        printf("\n");
    }
    km.BeforeShut();
    km.Shut();
    return 0;
}
