// resource_calls_plugin.cpp — NFCPropertyModule's resource calls through NFGPUKernelModule's seventeen
// named methods (include/NFGPUKernelModule.hpp) from a game-server-style client: the script of
// tests/resource_call_model.py (the golden world of tests/golden/resource_calls.json; the line formats are
// in tests/cpp/resource_calls_ref.cpp) replayed through the plugin API.  The Player's CommPropertyValue
// record (7 rows x MAXHP, MAXMP, MAXSP) is linked over all its rows; an object starts as the reference's
// module leaves it after CreateObject: every row used, row 0 the BASE values, HP / MP / SP full.  The
// module's other calls are made as a client makes them: SV a SetRecordInt on the group's row, LV (the level
// callback) one SetRecordInt on row 0 per column, then FullHPMP and FullSP, SP a SetPropertyInt.
// Every call line prints, in resource_calls_ref.cpp's format,
//   A <k> <ret> : <GetPropertyInt of HP MP SP MAXHP MAXMP MAXSP Gold Money of object o>
// (mid-window: the values as the reference holds them right after the call), every frame ("X") prints
//   F <window> <o> : <the same eight properties of every object after the frame>
// and every property event the frame delivers to the common property callback
//   P <window> <object> <name> <old> <new>
//
// usage: resource_calls_plugin <script.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
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
    int n_obj = 0;
    long long base[3] = {0, 0, 0};
    size_t at = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        if (f[0] == "BASE" && f.size() == 4) {
            for (int c = 0; c < 3; c++) base[c] = strtoll(f[1 + (size_t)c].c_str(), nullptr, 10);
        } else if (f[0] == "OBJ") {
            n_obj = atoi(f[1].c_str());
        } else {
            break;
        }
    }
    if (n_obj <= 0) return 2;
    const int rows = 7, cols = 3;
    const std::vector<std::string> tags = {"MAXHP", "MAXMP", "MAXSP"};
    const std::vector<std::string> names = {"HP", "MP", "SP", "MAXHP", "MAXMP", "MAXSP", "Gold", "Money"};
    const std::string rec = "CommPropertyValue";
    NFGPUKernelModule km(n_obj + 8);
    km.SetTimeSource([] { return g_now; });
    km.AddClass("Player");
    for (auto& nm : names) {
        km.AddProperty(nm, TDATA_INT);
        km.SetPropertyFlags("Player", nm, true, true, false);
    }
    km.AddRecord(rec, rows, std::vector<TDATA_TYPE>((size_t)cols, TDATA_INT));
    km.SetRecordFlags("Player", rec, false, true, false);
    km.LinkRecordColumns(rec, rows, tags);
    km.Init();
    km.CreateScene(1);
    auto guid = [&](int o) { return NFGUID(7, 100 + o); };
    std::vector<uint64_t> cells((size_t)rows * cols, 0);  // [cols][rows]: row 0 the base values
    std::map<std::string, TData> init;
    for (int c = 0; c < cols; c++) {
        cells[(size_t)c * rows] = (uint64_t)base[c];
        TData t;
        t.type = TDATA_INT;
        t.i = base[c];
        init[tags[(size_t)c]] = t;
        init[names[(size_t)c]] = t;  // (the level callback at creation filled HP, MP, SP)
    }
    for (int o = 0; o < n_obj; o++) {
        if (!km.CreateObject(guid(o), 1, 1 + o % 3, "Player", init)) return 3;
        if (!km.SetCreationRecord(guid(o), rec, (1ull << rows) - 1, cells)) return 3;
    }
    km.RegisterCommonPropertyEvent([&](const NFGUID& self, const std::string& name, const TData& o, const TData& n) {
        printf("P %d %d %s %lld %lld\n", g_window, (int)(self.nData64 - 100), name.c_str(), (long long)o.i, (long long)n.i);
        return 0;
    });
    km.AfterInit();
    auto print_props = [&](const NFGUID& g) {
        for (auto& nm : names) printf(" %lld", (long long)km.GetPropertyInt(g, nm));
        printf("\n");
    };

    int k = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        const std::string& op = f[0];
        if (op == "X") {
            g_now += 100;
            km.Execute();
            for (int o = 0; o < n_obj; o++) {
                printf("F %d %d :", g_window, o);
                print_props(guid(o));
            }
            g_window++;
            continue;
        }
        const NFGUID g = guid(atoi(f[1].c_str()));
        const int64_t v = f.size() > 2 ? strtoll(f[2].c_str(), nullptr, 10) : 0;
        long long ret = 0;
        if (op == "SV") {
            int col = 0;
            while (col < cols && tags[(size_t)col] != f[3]) col++;
            ret = km.SetRecordInt(g, rec, atoi(f[2].c_str()), col, (int)strtoll(f[4].c_str(), nullptr, 10));
        } else if (op == "LV") {
            ret = 1;
            for (int c = 0; c < cols; c++)
                ret = ret && km.SetRecordInt(g, rec, 0, c, (int)strtoll(f[3 + (size_t)c].c_str(), nullptr, 10));
            km.FullHPMP(g);
            km.FullSP(g);
        } else if (op == "SP") {
            ret = km.SetPropertyInt(g, f[2], strtoll(f[3].c_str(), nullptr, 10));
        } else if (op == "FullHPMP") ret = km.FullHPMP(g);
        else if (op == "FullSP") ret = km.FullSP(g);
        else if (op == "AddHP") ret = km.AddHP(g, v);
        else if (op == "ConsumeHP") ret = km.ConsumeHP(g, v);
        else if (op == "EnoughHP") ret = km.EnoughHP(g, v);
        else if (op == "AddMP") ret = km.AddMP(g, v);
        else if (op == "ConsumeMP") ret = km.ConsumeMP(g, v);
        else if (op == "EnoughMP") ret = km.EnoughMP(g, v);
        else if (op == "AddSP") ret = km.AddSP(g, v);
        else if (op == "ConsumeSP") ret = km.ConsumeSP(g, v);
        else if (op == "EnoughSP") ret = km.EnoughSP(g, v);
        else if (op == "AddMoney") ret = km.AddMoney(g, v);
        else if (op == "ConsumeMoney") ret = km.ConsumeMoney(g, v);
        else if (op == "EnoughMoney") ret = km.EnoughMoney(g, v);
        else if (op == "AddDiamond") ret = km.AddDiamond(g, v);
        else if (op == "ConsumeDiamond") ret = km.ConsumeDiamond(g, v);
        else if (op == "EnoughDiamond") ret = km.EnoughDiamond(g, v);
        else {
            fprintf(stderr, "bad script line %zu\n", at);
            return 2;
        }
        printf("A %d %lld :", k++, ret);
        print_props(g);
    }
    km.BeforeShut();
    km.Shut();
    return 0;
}
