// enter_snapshot_plugin.cpp — the enter views of NFGPUKernelModule (include/NFGPUKernelModule.hpp) from a
// game-server-style client: the script of tests/enter_snapshot_model.py (the golden world of
// tests/golden/enter_snapshot.json: PROP / REC / OBJ lines, then windows of SetProperty* and record calls
// with snapshot lines "S <obj> <view>" between them, "X" the frame) is replayed through the plugin API.
// The snapshots before a window's "X" see calls the library still holds queued (answered on the host),
// the snapshots after it the device's state.  Every snapshot prints, in the format of
// tests/cpp/enter_snapshot_ref.cpp,
//   V <k> <n props> <n records>
//   P <name> <bits> [<head>]
//   R <name> <used mask> : <cells, used rows ascending x columns>
// which tests/test_gpu_enter_snapshot.py compares with the recorded answers of the compiled reference.
// Then a GetGroupEnterViews case on a three-group world, checked here: "GROUP OK" or a non-zero exit.
//
// usage: enter_snapshot_plugin <script.txt>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "NFGPUKernelModule.hpp"

using namespace nfgpu;

static int64_t g_now = 0;

struct PropDef {
    std::string name;
    char type;
    int flags;
};
struct RecDef {
    std::string name, types;
    int rows, flags;
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

static uint64_t bits_of(const TData& d) {
    uint64_t b = (uint64_t)d.i;
    if (d.type == TDATA_FLOAT) memcpy(&b, &d.f, 8);
    return b;
}

static void print_view(int k, const NFGPUKernelModule::EnterView& v) {
    printf("V %d %zu %zu\n", k, v.properties.size(), v.records.size());
    for (auto& p : v.properties) {
        if (p.value.type == TDATA_OBJECT)
            printf("P %s %llu %llu\n", p.name->c_str(), (unsigned long long)(uint64_t)p.value.o.nData64,
                   (unsigned long long)(uint64_t)p.value.o.nHead64);
        else
            printf("P %s %llu\n", p.name->c_str(), (unsigned long long)bits_of(p.value));
    }
    for (auto& r : v.records) {
        printf("R %s %llu :", r.name->c_str(), (unsigned long long)r.used);
        for (auto& c : r.cells) printf(" %llu", (unsigned long long)bits_of(c));
        printf("\n");
    }
}

#define EXPECT(x)                                                       \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "group case: %s (line %d)\n", #x, __LINE__); \
            return 4;                                                   \
        }                                                               \
    } while (0)

// self arriving in (scene, group) of a three-group world: list order, self left out, self's own view
// last, an unknown group false
static int group_case() {
    NFGPUKernelModule km(64);
    km.SetTimeSource([] { return g_now; });
    km.AddProperty("HP", TDATA_INT);
    km.AddProperty("Name", TDATA_INT);
    km.AddProperty("Secret", TDATA_INT);
    km.AddClass("Player");
    km.AddClass("NPC");
    for (const char* c : {"Player", "NPC"}) {
        km.SetPropertyFlags(c, "HP", true, true, false);
        km.SetPropertyFlags(c, "Name", true, false, false);
        km.SetPropertyFlags(c, "Secret", false, true, false);
    }
    km.AddRecord("Bag", 4, {TDATA_INT});
    km.SetRecordFlags("Player", "Bag", true, false, false);
    km.SetRecordFlags("NPC", "Bag", false, true, false);
    km.Init();
    km.CreateScene(1);
    // groups 1..3; in group 2: players 20, 22, 24 and NPCs 21, 23 (NFGUID data halves)
    for (int o = 0; o < 30; o++) {
        const int group = o < 10 ? 1 : (o >= 20 && o < 25 ? 2 : 3);
        const bool player = group != 2 ? (o % 3 == 0) : (o % 2 == 0);
        TData hp, nm, se;
        hp.type = nm.type = se.type = TDATA_INT;
        hp.i = 100 + o;
        nm.i = o == 23 ? 0 : 1000 + o;
        se.i = 5;
        if (!km.CreateObject(NFGUID(7, o), 1, group, player ? "Player" : "NPC", {{"HP", hp}, {"Name", nm}, {"Secret", se}}))
            return 3;
    }
    km.AfterInit();
    g_now += 100;
    km.Execute();
    const NFGUID self(7, 22);
    std::vector<NFGUID> players, objects;
    std::vector<NFGPUKernelModule::EnterView> out;
    EXPECT(km.GetGroupEnterViews(self, 1, 2, players, objects, out));
    EXPECT(players.size() == 2 && players[0] == NFGUID(7, 20) && players[1] == NFGUID(7, 24));
    EXPECT(objects.size() == 4 && objects[0] == NFGUID(7, 20) && objects[1] == NFGUID(7, 24) &&
           objects[2] == NFGUID(7, 21) && objects[3] == NFGUID(7, 23));  // players, then the others, by NFGUID
    EXPECT(out.size() == 5);
    for (size_t i = 0; i < 4; i++) EXPECT(out[i].self == objects[i] && !out[i].bPrivate);
    EXPECT(out[4].self == self && !out[4].bPrivate);  // self's public view, for the players, last
    for (size_t i = 0; i < 5; i++) {
        const int o = (int)out[i].self.nData64;
        const bool npc23 = o == 23;  // (its Name is 0: not packed)
        EXPECT(out[i].properties.size() == (npc23 ? 1u : 2u));
        EXPECT(*out[i].properties[0].name == "HP" && out[i].properties[0].value.i == 100 + o);
        if (!npc23) EXPECT(*out[i].properties[1].name == "Name" && out[i].properties[1].value.i == 1000 + o);
        EXPECT(out[i].records.size() == (o % 2 == 0 ? 1u : 0u));  // the Bag is public for players only
    }
    // mid-window: a queued Set is in the view
    km.SetPropertyInt(NFGUID(7, 21), "Name", 0);
    EXPECT(km.GetGroupEnterViews(self, 1, 2, players, objects, out));
    EXPECT(out[2].self == NFGUID(7, 21) && out[2].properties.size() == 1);
    // self is no member yet (it arrives from group 3): nothing to leave out
    EXPECT(km.GetGroupEnterViews(NFGUID(7, 27), 1, 2, players, objects, out));
    EXPECT(players.size() == 3 && objects.size() == 5 && out.size() == 6 && out[5].self == NFGUID(7, 27));
    EXPECT(!km.GetGroupEnterViews(self, 1, 9, players, objects, out) && out.empty() && objects.empty());
    EXPECT(!km.GetGroupEnterViews(self, 5, 1, players, objects, out));
    // an object the module does not have: an empty view with a null self
    km.GetEnterViews({NFGUID(7, 20), NFGUID(9, 9), NFGUID(7, 20)}, {1, 0, 0}, out);
    EXPECT(out.size() == 3 && out[1].self.IsNull() && out[1].properties.empty() && out[1].records.empty());
    EXPECT(out[0].bPrivate && out[0].properties.size() == 2 && *out[0].properties[1].name == "Secret");
    EXPECT(out[0].records.empty() && out[2].records.size() == 1 && out[2].records[0].used == 0);
    km.BeforeShut();
    km.Shut();
    printf("GROUP OK\n");
    return 0;
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
    std::vector<PropDef> pdefs;
    std::vector<RecDef> rdefs;
    int n_obj = 0;
    for (auto& f : lines) {
        if (f[0] == "PROP") pdefs.push_back({f[1], f[2][0], atoi(f[3].c_str())});
        if (f[0] == "REC") rdefs.push_back({f[1], f[3], atoi(f[2].c_str()), atoi(f[4].c_str())});
        if (f[0] == "OBJ") n_obj = atoi(f[1].c_str());
    }
    {
        NFGPUKernelModule km(n_obj + 8);
        km.SetTimeSource([] { return g_now; });
        km.AddClass("Player");
        for (auto& d : pdefs) {
            km.AddProperty(d.name, d.type == 'I' ? TDATA_INT : d.type == 'F' ? TDATA_FLOAT : TDATA_OBJECT);
            km.SetPropertyFlags("Player", d.name, (d.flags & 1) != 0, (d.flags & 2) != 0, (d.flags & 4) != 0);
        }
        for (auto& d : rdefs) {
            std::vector<TDATA_TYPE> t;
            for (char c : d.types) t.push_back(c == 'I' ? TDATA_INT : TDATA_FLOAT);
            km.AddRecord(d.name, d.rows, t);
            km.SetRecordFlags("Player", d.name, (d.flags & 1) != 0, (d.flags & 2) != 0, (d.flags & 4) != 0);
        }
        km.Init();
        km.CreateScene(1);
        auto guid = [&](int o) { return NFGUID(7, 100 + o); };
        for (int o = 0; o < n_obj; o++)
            if (!km.CreateObject(guid(o), 1, 1 + o % 3, "Player")) return 3;
        km.AfterInit();
        auto types_of = [&](const std::string& rec) -> const std::string& {
            for (auto& d : rdefs)
                if (d.name == rec) return d.types;
            return rdefs[0].types;
        };
        int k = 0;
        std::vector<NFGPUKernelModule::EnterView> out;
        for (auto& f : lines) {
            const std::string& op = f[0];
            if (op == "PROP" || op == "REC" || op == "OBJ") continue;
            if (op == "X") {
                g_now += 100;
                km.Execute();
                continue;
            }
            const NFGUID g = guid(atoi(f[1].c_str()));
            if (op == "SI") {
                km.SetPropertyInt(g, f[2], strtoll(f[3].c_str(), nullptr, 10));
            } else if (op == "SF") {
                km.SetPropertyFloat(g, f[2], strtod(f[3].c_str(), nullptr));
            } else if (op == "SO") {
                km.SetPropertyObject(g, f[2], NFGUID(strtoll(f[3].c_str(), nullptr, 10), strtoll(f[4].c_str(), nullptr, 10)));
            } else if (op == "S") {
                km.GetEnterViews({g}, {(uint8_t)(f[2] == "1")}, out);
                print_view(k++, out[0]);
            } else if (op == "AR") {
                std::vector<TData> v;
                for (size_t c = 0; c + 4 < f.size(); c++) v.push_back(value_of(types_of(f[2])[c], f[4 + c]));
                km.AddRow(g, f[2], atoi(f[3].c_str()), v);
            } else if (op == "RI") {
                km.SetRecordInt(g, f[2], atoi(f[3].c_str()), atoi(f[4].c_str()), strtoll(f[5].c_str(), nullptr, 10));
            } else if (op == "RM") {
                km.RemoveRow(g, f[2], atoi(f[3].c_str()));
            } else if (op == "CL") {
                km.ClearRecord(g, f[2]);
            } else {
                fprintf(stderr, "bad script line: %s\n", op.c_str());
                return 2;
            }
        }
        km.BeforeShut();
        km.Shut();
    }
    return group_case();
}
